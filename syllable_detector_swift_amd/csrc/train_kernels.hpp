// train_kernels.hpp -- the text of the training kernels (kernels_train.hip has the notes): the gradient, the range and the two combine
// kernels as templates whose trailing parameter pack holds the multi form's extra arguments.  kernels_train.hip instantiates the plain
// forms (no pack) and kernels_train_multi.hip the multi forms (syldet_trainer_create_multi), each into a code object of its own.
// Everything here is in an anonymous namespace inside sd: each of the two files gets its own instantiations.

#pragma once

#include "generic_eval.hpp"
#include "train_targets.hpp"

namespace sd {

namespace {

constexpr int kWave = 64;

__device__ __forceinline__ float transfer_slope(int tf, float h)
{
    switch (tf) {
    case 0: return 1.0f - h * h;                               // TanSig
    case 1: return h * (1.0f - h);                             // LogSig
    case 3: return h > 0.0f && h < 1.0f ? 1.0f : 0.0f;         // SatLin: 0 < a < 1, where h = a
    default: return 1.0f;                                      // PureLin
    }
}

// One input function on one element, in the generic engine's operations: the normalisers with their statistics (a, b, c), the maps
// with their own offset and gain.  l2normalize v / s and normalizestd (v - mean) / sd; normalize v slope + intercept (range 0:
// slope 0 and intercept -1, the engine's fill) and the maps (v - xOffset) gain + y.
__device__ __forceinline__ float apply_fn(int kind, float v, float a, float b, float c)
{
    return kind == 0 || kind == 2 ? (v - a) / b : (v - a) * b + c;
}

// The input chain of one evaluation, ONE TEXT for train_gradient_kernel and train_range_kernel, as macros that are expanded inside the
// kernels and not as functions: written as __forceinline__ functions (with the statistics in a struct, or in three arrays passed
// by reference) the same statements gave the same bits but compiled to another instruction stream for the gradient kernel -- 15 %
// more instructions in its inner loops, 31.3 -> 34.8 ms a gradient on the archive of MEASUREMENTS "Training" -- whereas expanded in
// place the gradient kernel's code is instruction for instruction what it was before the range kernel shared it.  They use the
// kernels' own names: d, cols, row, row_stride, e0, n, tid, NT, F, FP, T, I, stage; mine_rows, sa, sb, sc; stats, KS, xo, gn.
//   SD_TRAIN_STAGE_TILE    the tile's n + T - 1 frames into LDS, scaled (linear / log / dB)
//   SD_TRAIN_CHAIN_VALUE   defines value(t, f, upto): element (t, f) behind the input functions in front of `upto`
//   SD_TRAIN_CHAIN_STATS   the statistics sa, sb, sc of the input functions in front of UPTO, in file order (l2normalize: frame sums,
//                          then their sum; normalize: a range of 0 fills -1; normalizestd: the population sigma; a map: its y)
//   SD_TRAIN_CHAIN_AT      V, the staged element of evaluation E at the thread's input position, through the functions in front of UPTO
#define SD_TRAIN_STAGE_TILE()                                                  \
    {                                                                          \
        const float *src = cols + (int64_t)row * row_stride + e0 * F;          \
        const unsigned total = (unsigned)(n + T - 1) * (unsigned)F;            \
        for (unsigned idx = (unsigned)tid; idx < total; idx += (unsigned)NT) { \
            const unsigned fr = idx / (unsigned)F, f = idx - fr * (unsigned)F; \
            float v = src[idx];                                                \
            if (d.scaling == 1) v = logf(v);                                   \
            else if (d.scaling == 2) v = 20.0f * log10f(v);                    \
            stage[fr * FP + f] = v;                                            \
        }                                                                      \
    }

#define SD_TRAIN_CHAIN_VALUE()                                 \
    auto value = [&](int t, int f, int upto) {                 \
        float v = mine_rows[t * FP + f];                       \
    _Pragma("unroll")                                          \
        for (int kk = 0; kk < kMaxFns; kk++) {                 \
            if (kk < upto) {                                   \
                const int kind = d.in_fns[kk].kind;            \
                float a = sa[kk], b = sb[kk];                  \
                if (kind >= 3) {                               \
                    a = d.maps[d.in_fns[kk].xoff + t * F + f]; \
                    b = d.maps[d.in_fns[kk].gain + t * F + f]; \
                }                                              \
                v = apply_fn(kind, v, a, b, sc[kk]);           \
            }                                                  \
        }                                                      \
        return v;                                              \
    };

#define SD_TRAIN_CHAIN_STATS(UPTO)                                    \
    _Pragma("unroll")                                                 \
    for (int k = 0; k < kMaxFns; k++) {                               \
        if (k < (UPTO)) {                                             \
            const int kind = d.in_fns[k].kind;                        \
            if (kind == 0) {                                          \
                float s = 0.0f;                                       \
                for (int t = 0; t < T; t++) {                         \
                    float fs = 0.0f;                                  \
                    for (int f = 0; f < F; f++) {                     \
                        const float v = value(t, f, k);               \
                        fs = fmaf(v, v, fs);                          \
                    }                                                 \
                    s += fs;                                          \
                }                                                     \
                sb[k] = sqrtf(s);                                     \
            } else if (kind == 1) {                                   \
                float mn = INFINITY, mx = -INFINITY;                  \
                for (int t = 0; t < T; t++)                           \
                    for (int f = 0; f < F; f++) {                     \
                        const float v = value(t, f, k);               \
                        mn = fminf(mn, v);                            \
                        mx = fmaxf(mx, v);                            \
                    }                                                 \
                const float range = mx - mn;                          \
                if (range == 0.0f) {                                  \
                    sb[k] = 0.0f;                                     \
                    sc[k] = -1.0f;                                    \
                } else {                                              \
                    sb[k] = 2.0f / range;                             \
                    sc[k] = (0.0f - mn - mx) / range;                 \
                }                                                     \
            } else if (kind == 2) {                                   \
                float s = 0.0f;                                       \
                for (int t = 0; t < T; t++) {                         \
                    float fs = 0.0f;                                  \
                    for (int f = 0; f < F; f++) fs += value(t, f, k); \
                    s += fs;                                          \
                }                                                     \
                const float mean = s / (float)I;                      \
                float q = 0.0f;                                       \
                for (int t = 0; t < T; t++) {                         \
                    float fq = 0.0f;                                  \
                    for (int f = 0; f < F; f++) {                     \
                        const float dl = value(t, f, k) - mean;       \
                        fq = fmaf(dl, dl, fq);                        \
                    }                                                 \
                    q += fq;                                          \
                }                                                     \
                sa[k] = mean;                                         \
                sb[k] = sqrtf(q / (float)I);                          \
            } else {                                                  \
                sc[k] = d.in_fns[k].y;                                \
            }                                                         \
        }                                                             \
    }

#define SD_TRAIN_CHAIN_AT(V, UPTO, E)                                                        \
    _Pragma("unroll")                                                                        \
    for (int k = 0; k < kMaxFns; k++) {                                                      \
        if (k < (UPTO)) {                                                                    \
            const int kind = d.in_fns[k].kind;                                               \
            const float4 st = stats[(E) * KS + k];                                           \
            V = apply_fn(kind, V, kind >= 3 ? xo[k] : st.x, kind >= 3 ? gn[k] : st.y, st.z); \
        }                                                                                    \
    }

// The multi form's workgroup (blockIdx.x, blockIdx.y) = (g, n), ONE TEXT for the gradient and the range kernel: network n's rows,
// its G_n = min(its tiles, BOUND) workgroups (the others leave before anything is read), its own TrainDesc; then n_tiles is the
// network's, the stride over them G_n, and the partial n BOUND + g.  BOUND is what the plain form has in n_tiles' place.
// The multi form's extra arguments are a parameter pack at the end of each kernel: the plain instantiation has none, so its
// kernel arguments are the plain launch's alone, and no statement of the multi form is compiled into it (`if constexpr (MULTI)`).
template <class A, class... R> __device__ __forceinline__ const A &pack_first(const A &a, const R &...) { return a; }
template <class A, class B> __device__ __forceinline__ const B &pack_second(const A &, const B &b) { return b; }

#define SD_TRAIN_MULTI_GROUP(BOUND)                                                 \
    {                                                                               \
        const TrainMulti &mu = pack_first(multi...);                                \
        net = (int)blockIdx.y;                                                      \
        const int first_row = mu.net_row_begin[net];                                          \
        const int64_t mine_tiles = (int64_t)(mu.net_row_begin[net + 1] - first_row) * tiles_per_row; \
        const int bound = (BOUND);                                                  \
        step = (int)(mine_tiles < bound ? mine_tiles : bound);                      \
        if ((int)blockIdx.x >= step) return;                                        \
        d = mu.descs[net];                                                          \
        n_tiles = (int)mine_tiles;                                                  \
        slot = (int64_t)net * bound + (int64_t)blockIdx.x;                          \
        net_rows = mu.rows + first_row;                                             \
    }

template <int HP, class... MU>
__global__ void __launch_bounds__(512)
train_gradient_kernel(TrainDesc d, const float *__restrict__ cols, int64_t row_stride, const float *__restrict__ theta,
                      const float *__restrict__ targets, const float *__restrict__ weights, int64_t n_evals, int tiles_per_row, int n_tiles,
                      double *part, MU... multi)
{
    constexpr bool MULTI = sizeof...(MU) != 0;
    int net = 0, step = 0;                                     // (the multi form's stride over its network's tiles)
    int64_t slot = (int64_t)blockIdx.x;
    const int32_t *net_rows = nullptr;
    if constexpr (MULTI) SD_TRAIN_MULTI_GROUP(n_tiles)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x, lane = tid & (kWave - 1), wave = tid / kWave, waves = NT / kWave;
    const int F = d.F, T = d.T, I = d.I, H = d.H, O = d.O, FP = d.FP, K = d.n_in_fns, KS = K > 0 ? K : 1;
    const int S = H + O * H + O, P = H * I + S;
    const int ob1 = H * I, oW2 = ob1 + H, ob2 = oW2 + O * H;
    float *w1t = (float *)smem;                                // [I][HP]
    float *stage = (float *)(smem + d.lds_stage);              // [tile + T - 1][FP]
    float *d1s = (float *)(smem + d.lds_d1);                   // [tile][HP]
    float4 *stats = (float4 *)(smem + d.lds_stats);            // [tile][KS]
    double *red64 = (double *)(smem + d.lds_red);              // [waves][2]
    float *red32 = (float *)(red64 + 2 * waves);               // [waves][S]
    int *sel = (int *)(smem + d.lds_sel);                      // [tile]
    double *mine = part + slot * (P + 2);
    if constexpr (MULTI) theta += (int64_t)net * P;

    // the first layer transposed, and this workgroup's partial from +0: every entry by the thread that will add to it
    for (int idx = tid; idx < I * HP; idx += NT) {
        const int i = idx / HP, h = idx - i * HP;
        w1t[idx] = h < H ? theta[h * I + i] : 0.0f;
    }
    for (int i = tid; i < I; i += NT)
        for (int h = 0; h < H; h++) mine[h * I + i] = 0.0;
    if (tid < S + 2) mine[ob1 + tid] = 0.0;

    for (int tl = (int)blockIdx.x; tl < n_tiles; tl += MULTI ? step : (int)gridDim.x) {
        const int own_row = tl / tiles_per_row;
        const int row = MULTI ? net_rows[own_row] : own_row;
        const int64_t e0 = (int64_t)(tl - own_row * tiles_per_row) * d.tile;
        const int n = (int)(n_evals - e0 < d.tile ? n_evals - e0 : d.tile);
        __syncthreads();                                       // the last tile's LDS is read to the end
        float wgt = 0.0f;
        if (tid < n) wgt = weights[(int64_t)row * n_evals + e0 + tid];
        const bool active = wgt > 0.0f;                        // (a NaN weight is not selected)
        if (!__syncthreads_or(active ? 1 : 0)) continue;
        if (tid < d.tile) sel[tid] = active ? 1 : 0;
        SD_TRAIN_STAGE_TILE()
        __syncthreads();

        // ---- forward and the deltas: a thread an evaluation ----
        float h1[HP], d1[HP], d2[kTrainMaxOut];
        float sa[kMaxFns], sb[kMaxFns], sc[kMaxFns];
#pragma unroll
        for (int h = 0; h < HP; h++) h1[h] = d1[h] = 0.0f;
#pragma unroll
        for (int o = 0; o < kTrainMaxOut; o++) d2[o] = 0.0f;
#pragma unroll
        for (int k = 0; k < kMaxFns; k++) {
            sa[k] = 0.0f;
            sb[k] = 1.0f;
            sc[k] = 0.0f;
        }
        double loss = 0.0;
        if (active) {
            const float *mine_rows = stage + tid * FP;
            SD_TRAIN_CHAIN_VALUE()
            SD_TRAIN_CHAIN_STATS(K)
            // the first layer: a frame's products summed on their own, then the frames
            float acc[HP];
#pragma unroll
            for (int h = 0; h < HP; h++) acc[h] = 0.0f;
            for (int t = 0; t < T; t++) {
                float fa[HP];
#pragma unroll
                for (int h = 0; h < HP; h++) fa[h] = 0.0f;
                for (int f = 0; f < F; f++) {
                    const float v = value(t, f, K);
                    const float4 *wr = (const float4 *)(w1t + (t * F + f) * HP);
#pragma unroll
                    for (int q = 0; q < HP / 4; q++) {
                        const float4 w = wr[q];
                        fa[4 * q] = fmaf(w.x, v, fa[4 * q]);
                        fa[4 * q + 1] = fmaf(w.y, v, fa[4 * q + 1]);
                        fa[4 * q + 2] = fmaf(w.z, v, fa[4 * q + 2]);
                        fa[4 * q + 3] = fmaf(w.w, v, fa[4 * q + 3]);
                    }
                }
#pragma unroll
                for (int h = 0; h < HP; h++) acc[h] += fa[h];
            }
#pragma unroll
            for (int h = 0; h < HP; h++)
                if (h < H) h1[h] = generic_dev::transfer(d.tf0, acc[h] + theta[ob1 + h]);
            // the second layer, the reverse output maps, the loss term and the output deltas
            float term = 0.0f;
            const float *tg = targets + ((int64_t)row * n_evals + e0 + tid) * O;
#pragma unroll
            for (int o = 0; o < kTrainMaxOut; o++) {
                if (o < O) {
                    float a2 = 0.0f;
#pragma unroll
                    for (int h = 0; h < HP; h++)
                        if (h < H) a2 = fmaf(theta[oW2 + o * H + h], h1[h], a2);
                    const float h2 = generic_dev::transfer(d.tf1, a2 + theta[ob2 + o]);
                    float y = h2, slope = transfer_slope(d.tf1, h2);
#pragma unroll
                    for (int k = 0; k < kMaxFns; k++) {
                        if (k < d.n_out_fns) {
                            const float gain = d.maps[d.out_fns[k].gain + o];
                            y = (y - d.out_fns[k].y) / gain + d.maps[d.out_fns[k].xoff + o];
                            slope = slope / gain;
                        }
                    }
                    const float diff = y - tg[o];
                    term = fmaf(diff, diff, term);
                    d2[o] = 2.0f * wgt * diff * slope;
                }
            }
            loss = (double)(wgt * term);
#pragma unroll
            for (int h = 0; h < HP; h++) {
                if (h < H) {
                    float back = 0.0f;
#pragma unroll
                    for (int o = 0; o < kTrainMaxOut; o++)
                        if (o < O) back = fmaf(theta[oW2 + o * H + h], d2[o], back);
                    d1[h] = transfer_slope(d.tf0, h1[h]) * back;
                }
            }
        }
        if (tid < d.tile) {
#pragma unroll
            for (int q = 0; q < HP / 4; q++)
                ((float4 *)(d1s + tid * HP))[q] = make_float4(d1[4 * q], d1[4 * q + 1], d1[4 * q + 2], d1[4 * q + 3]);
#pragma unroll
            for (int k = 0; k < kMaxFns; k++)
                if (k < KS) stats[tid * KS + k] = make_float4(sa[k], sb[k], sc[k], 0.0f);
        }
        // ---- the small parameters, the loss and the weight sum: wave trees, then the waves in order ----
#pragma unroll
        for (int h = 0; h < HP; h++) {
            if (h < H) {
                const float s = generic_dev::wave_sum(d1[h]);
                if (lane == 0) red32[wave * S + h] = s;
            }
        }
#pragma unroll
        for (int o = 0; o < kTrainMaxOut; o++) {
            if (o < O) {
#pragma unroll
                for (int h = 0; h < HP; h++) {
                    if (h < H) {
                        const float s = generic_dev::wave_sum(d2[o] * h1[h]);
                        if (lane == 0) red32[wave * S + H + o * H + h] = s;
                    }
                }
                const float s = generic_dev::wave_sum(d2[o]);
                if (lane == 0) red32[wave * S + H + O * H + o] = s;
            }
        }
        {
            const double l = generic_dev::wave_sum_f64(loss), w = generic_dev::wave_sum_f64(active ? (double)wgt : 0.0);
            if (lane == 0) {
                red64[2 * wave] = l;
                red64[2 * wave + 1] = w;
            }
        }
        __syncthreads();
        if (tid < S) {
            float s = 0.0f;
            for (int wv = 0; wv < waves; wv++) s += red32[wv * S + tid];
            mine[ob1 + tid] += (double)s;
        } else if (tid < S + 2) {
            double s = 0.0;
            for (int wv = 0; wv < waves; wv++) s += red64[2 * wv + (tid - S)];
            mine[P + (tid - S)] += s;
        }

        // ---- dW1: a thread an input position, the tile's selected evaluations in order ----
        for (int i = tid; i < I; i += NT) {
            const int t = i / F, f = i - t * F;
            float xo[kMaxFns], gn[kMaxFns];
#pragma unroll
            for (int k = 0; k < kMaxFns; k++) {
                xo[k] = gn[k] = 0.0f;
                if (k < K && d.in_fns[k].kind >= 3) {
                    xo[k] = d.maps[d.in_fns[k].xoff + i];
                    gn[k] = d.maps[d.in_fns[k].gain + i];
                }
            }
            float acc[HP];
#pragma unroll
            for (int h = 0; h < HP; h++) acc[h] = 0.0f;
            const float *col = stage + t * FP + f;
            for (int e = 0; e < n; e++) {
                if (!sel[e]) continue;
                float v = col[e * FP];
                SD_TRAIN_CHAIN_AT(v, K, e)
                const float4 *dr = (const float4 *)(d1s + e * HP);
#pragma unroll
                for (int q = 0; q < HP / 4; q++) {
                    const float4 dl = dr[q];
                    acc[4 * q] = fmaf(dl.x, v, acc[4 * q]);
                    acc[4 * q + 1] = fmaf(dl.y, v, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(dl.z, v, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(dl.w, v, acc[4 * q + 3]);
                }
            }
#pragma unroll
            for (int h = 0; h < HP; h++)
                if (h < H) mine[h * I + i] += (double)acc[h];
        }
    }
}

// The multi form of the two combine kernels: blockIdx.y is the network; `groups` is the bound, and the network's own G_n follows from
// its rows as in SD_TRAIN_MULTI_GROUP.  The results move to the network's place.
#define SD_TRAIN_MULTI_COMBINE()                                                            \
    {                                                                                       \
        const TrainMulti &mu = pack_first(multi...);                                        \
        const int tiles_per_row = pack_second(multi...);                                    \
        const int net = (int)blockIdx.y;                                                    \
        const int64_t mine_tiles = (int64_t)(mu.net_row_begin[net + 1] - mu.net_row_begin[net]) * tiles_per_row; \
        part += (int64_t)net * groups * (P + 2);                                            \
        if (mine_tiles < groups) groups = (int)mine_tiles;                                  \
    }

template <class... MU>
__global__ void __launch_bounds__(256)
train_combine_kernel(int P, int groups, const double *__restrict__ part, double *__restrict__ loss, float *__restrict__ gradient, MU... multi)
{
    constexpr bool MULTI = sizeof...(MU) != 0;
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= P + 2) return;
    if constexpr (MULTI) {
        SD_TRAIN_MULTI_COMBINE()
        loss += 2 * (int64_t)blockIdx.y;
        gradient += (int64_t)blockIdx.y * P;
    }
    double s = 0.0;
    for (int g = 0; g < groups; g++) s = s + part[(int64_t)g * (P + 2) + p];
    if (p < P) gradient[p] = (float)s;
    else loss[p - P] = s;
}

// The input range (syldet_train_input_range_device): the gradient kernel's tiling and staging, the statistics and values of the
// functions in front of input function `at` by the gradient's own text (the SD_TRAIN_ macros above).  A workgroup's partial
// is float [2][I] (least, greatest) and an int64 count behind it, in the P + 2 doubles the gradient keeps a workgroup.
template <class... MU>
__global__ void __launch_bounds__(512)
train_range_kernel(TrainDesc d, int at, const float *__restrict__ cols, int64_t row_stride, const float *__restrict__ weights, int64_t n_evals,
                   int tiles_per_row, int n_tiles, double *part, MU... multi)
{
    constexpr bool MULTI = sizeof...(MU) != 0;
    int net = 0, step = 0;                                     // (the multi form's stride over its network's tiles)
    int64_t slot = (int64_t)blockIdx.x;
    const int32_t *net_rows = nullptr;
    if constexpr (MULTI) SD_TRAIN_MULTI_GROUP(n_tiles)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int F = d.F, T = d.T, I = d.I, FP = d.FP, K = d.n_in_fns, KS = K > 0 ? K : 1;
    const int P = d.H * I + d.H + d.O * d.H + d.O;
    float *stage = (float *)(smem + d.lds_stage);              // [tile + T - 1][FP]
    float4 *stats = (float4 *)(smem + d.lds_stats);            // [tile][KS]
    int *sel = (int *)(smem + d.lds_sel);                      // [tile]
    float *mine = (float *)(part + slot * (P + 2));
    for (int i = tid; i < I; i += NT) {
        mine[i] = INFINITY;
        mine[I + i] = -INFINITY;
    }
    int64_t count = 0;
    for (int tl = (int)blockIdx.x; tl < n_tiles; tl += MULTI ? step : (int)gridDim.x) {
        const int own_row = tl / tiles_per_row;
        const int row = MULTI ? net_rows[own_row] : own_row;
        const int64_t e0 = (int64_t)(tl - own_row * tiles_per_row) * d.tile;
        const int n = (int)(n_evals - e0 < d.tile ? n_evals - e0 : d.tile);
        __syncthreads();                                       // the last tile's LDS is read to the end
        float wgt = 0.0f;
        if (tid < n) wgt = weights[(int64_t)row * n_evals + e0 + tid];
        const bool active = wgt > 0.0f;                        // (a NaN weight is not selected)
        if (!__syncthreads_or(active ? 1 : 0)) continue;
        SD_TRAIN_STAGE_TILE()
        __syncthreads();

        // ---- a thread an evaluation: the statistics in front of the map, and whether all I values there are finite ----
        float sa[kMaxFns], sb[kMaxFns], sc[kMaxFns];
#pragma unroll
        for (int k = 0; k < kMaxFns; k++) {
            sa[k] = 0.0f;
            sb[k] = 1.0f;
            sc[k] = 0.0f;
        }
        bool whole = false;
        if (active) {
            const float *mine_rows = stage + tid * FP;
            SD_TRAIN_CHAIN_VALUE()
            SD_TRAIN_CHAIN_STATS(at)
            whole = true;
            for (int t = 0; t < T; t++)
                for (int f = 0; f < F; f++) whole = whole && isfinite(value(t, f, at));
        }
        if (tid < d.tile) {
            sel[tid] = whole ? 1 : 0;
#pragma unroll
            for (int k = 0; k < kMaxFns; k++)
                if (k < KS) stats[tid * KS + k] = make_float4(sa[k], sb[k], sc[k], 0.0f);
        }
        const int contributing = __syncthreads_count(whole ? 1 : 0);
        count += contributing;
        if (!contributing) continue;

        // ---- a thread an input position: the tile's contributing evaluations ----
        for (int i = tid; i < I; i += NT) {
            const int t = i / F, f = i - t * F;
            float xo[kMaxFns], gn[kMaxFns];
#pragma unroll
            for (int k = 0; k < kMaxFns; k++) {
                xo[k] = gn[k] = 0.0f;
                if (k < at && d.in_fns[k].kind >= 3) {
                    xo[k] = d.maps[d.in_fns[k].xoff + i];
                    gn[k] = d.maps[d.in_fns[k].gain + i];
                }
            }
            float mn = INFINITY, mx = -INFINITY;
            const float *col = stage + t * FP + f;
            for (int e = 0; e < n; e++) {
                if (!sel[e]) continue;
                float v = col[e * FP];
                SD_TRAIN_CHAIN_AT(v, at, e)
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
            mine[i] = fminf(mine[i], mn);
            mine[I + i] = fmaxf(mine[I + i], mx);
        }
    }
    if (tid == 0) *(int64_t *)(mine + 2 * I) = count;
}

// A thread an input position: the least and the greatest over the G partials (a zero as +0.0); thread 0 adds the counts.
template <class... MU>
__global__ void __launch_bounds__(256)
train_range_combine_kernel(int I, int P, int groups, const double *__restrict__ part, float *__restrict__ range, int64_t *__restrict__ count, MU... multi)
{
    constexpr bool MULTI = sizeof...(MU) != 0;
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= I) return;
    if constexpr (MULTI) {
        SD_TRAIN_MULTI_COMBINE()
        range += 2 * (int64_t)blockIdx.y * I;
        count += blockIdx.y;
    }
    float mn = INFINITY, mx = -INFINITY;
    int64_t c = 0;
    for (int g = 0; g < groups; g++) {
        const float *one = (const float *)(part + (int64_t)g * (P + 2));
        mn = fminf(mn, one[i]);
        mx = fmaxf(mx, one[I + i]);
        if (i == 0) c += *(const int64_t *)(one + 2 * I);
    }
    range[i] = mn == 0.0f ? 0.0f : mn;
    range[I + i] = mx == 0.0f ? 0.0f : mx;
    if (i == 0) *count = c;
}

}  // namespace

}  // namespace sd
