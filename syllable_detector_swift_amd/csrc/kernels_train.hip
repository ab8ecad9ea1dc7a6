// kernels_train.hip -- training (syldet_train_targets_device, syldet_train_gradient_device of include/syldet.h): targets and class
// weights from labels, and loss and gradient of a two-layer network's parameters over weighted evaluations, taken straight from the
// spectrogram columns.  The N x I input matrix (the columns repeated timeRange times) is never formed.
//
//   train_targets_kernel   A thread an element of weights [rows][n_evals]: its detector (the row, or a search of the row's
//                  recordings), then train_targets.hpp, the text the host runs.  Every element is written.
//   train_gradient_kernel  Workgroup g of G takes the tiles g, g + G, ... in order; a tile is `tile` consecutive evaluations of one row.
//                  A tile without a selected evaluation (w > 0) is left before anything of it is read.  Else its tile + T - 1 frames
//                  are staged in LDS once, scaled (linear / log / dB), rows padded to an odd length.  Then
//                    forward    a thread owns an evaluation: the normalisers' statistics, the first layer against the transposed
//                               weights in LDS (one broadcast 16-byte read for four units), the second layer, the reverse output
//                               maps, the loss term and the two layers' deltas -- in registers.  An unselected evaluation computes
//                               nothing and leaves zeros: selection, not a product with zero.
//                    small      b1, W2, b2, loss and weight sum: fixed wave trees, the waves' results added in wave order.
//                    dW1        a thread owns the input position i (all hidden units) and walks the tile's selected evaluations in
//                               order: the processed input is recomputed from the staged frames and the evaluation's statistics,
//                               one multiply-add a hidden unit, fp32.
//                  Each tile's sums go into the workgroup's fp64 partial in global memory, every entry by the one thread that owns
//                  it: no atomics, and the order is a function of the shapes alone.
//   train_combine_kernel   A thread a parameter: the G partials added in group order in fp64, rounded once to fp32.
//   train_range_kernel     The same tiles, staged the same way: a thread an evaluation makes the statistics of the input functions in
//                  front of the first mapminmax and decides whether all I values there are finite; then a thread an input position
//                  takes the least and the greatest over the tile's contributing evaluations into the workgroup's partial.  The
//                  staging, the statistics and the values are the gradient kernel's own text (the SD_TRAIN_ macros).
//   train_range_combine_kernel   A thread an input position: least and greatest over the G partials; the counts added.
//
// gfx950 only: wave = 64 lanes.  Plain HIP C++, vector loads and stores, no float atomics.

#include "generic_eval.hpp"
#include "train_targets.hpp"

namespace sd {

namespace {

constexpr int kWave = 64;
constexpr int kTargetsThreads = 256;
constexpr int kLdsComfort = 72 * 1024;       // two workgroups a CU
constexpr int kLdsLimit = 150 * 1024;

__global__ void __launch_bounds__(kTargetsThreads)
train_targets_kernel(TrainTargetsDesc d, int64_t n_evals, float *__restrict__ targets, float *__restrict__ weights)
{
    const int64_t e = (int64_t)blockIdx.x * kTargetsThreads + threadIdx.x;
    const int row = (int)blockIdx.y;
    if (e >= n_evals) return;
    int det = row;
    int64_t own = e;
    bool has = true;
    if (d.dets) {
        // the last detector of the row that starts at or before e
        int lo = d.row_begin[row], hi = d.row_begin[row + 1];
        const int first = lo;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (d.dets[mid].first_eval <= e) lo = mid + 1;
            else hi = mid;
        }
        has = lo > first && e - d.dets[lo - 1].first_eval < d.dets[lo - 1].n_evals;
        if (has) {
            det = d.dets[lo - 1].det;
            own = e - d.dets[lo - 1].first_eval;
        }
    }
    uint32_t mask = 0;
    if (has) {
        const int64_t b0 = d.label_begin[det], b1 = d.label_begin[det + 1];
        mask = train_target_mask(d.first_index + own * d.hop, d.labels + b0, d.label_output ? d.label_output + b0 : nullptr, b1 - b0, d.half_width);
    }
    float t[kTrainMaxOut], w;
    train_target_write(mask, d.n_out, d.weight_positive, d.weight_negative, t, &w);
    const int64_t at = (int64_t)row * n_evals + e;
    for (int o = 0; o < d.n_out; o++) targets[at * d.n_out + o] = has ? t[o] : 0.0f;
    weights[at] = has ? w : 0.0f;
}

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

template <int HP>
__global__ void __launch_bounds__(512)
train_gradient_kernel(TrainDesc d, const float *__restrict__ cols, int64_t row_stride, const float *__restrict__ theta,
                      const float *__restrict__ targets, const float *__restrict__ weights, int64_t n_evals, int tiles_per_row, int n_tiles,
                      double *part)
{
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
    double *mine = part + (int64_t)blockIdx.x * (P + 2);

    // the first layer transposed, and this workgroup's partial from +0: every entry by the thread that will add to it
    for (int idx = tid; idx < I * HP; idx += NT) {
        const int i = idx / HP, h = idx - i * HP;
        w1t[idx] = h < H ? theta[h * I + i] : 0.0f;
    }
    for (int i = tid; i < I; i += NT)
        for (int h = 0; h < H; h++) mine[h * I + i] = 0.0;
    if (tid < S + 2) mine[ob1 + tid] = 0.0;

    for (int tl = (int)blockIdx.x; tl < n_tiles; tl += (int)gridDim.x) {
        const int row = tl / tiles_per_row;
        const int64_t e0 = (int64_t)(tl - row * tiles_per_row) * d.tile;
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

__global__ void __launch_bounds__(256)
train_combine_kernel(int P, int groups, const double *__restrict__ part, double *__restrict__ loss, float *__restrict__ gradient)
{
    const int p = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (p >= P + 2) return;
    double s = 0.0;
    for (int g = 0; g < groups; g++) s = s + part[(int64_t)g * (P + 2) + p];
    if (p < P) gradient[p] = (float)s;
    else loss[p - P] = s;
}

// The input range (syldet_train_input_range_device): the gradient kernel's tiling and staging, the statistics and values of the
// functions in front of input function `at` by the gradient's own text (the SD_TRAIN_ macros above).  A workgroup's partial
// is float [2][I] (least, greatest) and an int64 count behind it, in the P + 2 doubles the gradient keeps a workgroup.
__global__ void __launch_bounds__(512)
train_range_kernel(TrainDesc d, int at, const float *__restrict__ cols, int64_t row_stride, const float *__restrict__ weights, int64_t n_evals,
                   int tiles_per_row, int n_tiles, double *part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, NT = (int)blockDim.x;
    const int F = d.F, T = d.T, I = d.I, FP = d.FP, K = d.n_in_fns, KS = K > 0 ? K : 1;
    const int P = d.H * I + d.H + d.O * d.H + d.O;
    float *stage = (float *)(smem + d.lds_stage);              // [tile + T - 1][FP]
    float4 *stats = (float4 *)(smem + d.lds_stats);            // [tile][KS]
    int *sel = (int *)(smem + d.lds_sel);                      // [tile]
    float *mine = (float *)(part + (int64_t)blockIdx.x * (P + 2));
    for (int i = tid; i < I; i += NT) {
        mine[i] = INFINITY;
        mine[I + i] = -INFINITY;
    }
    int64_t count = 0;
    for (int tl = (int)blockIdx.x; tl < n_tiles; tl += (int)gridDim.x) {
        const int row = tl / tiles_per_row;
        const int64_t e0 = (int64_t)(tl - row * tiles_per_row) * d.tile;
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
__global__ void __launch_bounds__(256)
train_range_combine_kernel(int I, int P, int groups, const double *__restrict__ part, float *__restrict__ range, int64_t *__restrict__ count)
{
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (i >= I) return;
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

int up16(int n) { return (n + 15) / 16 * 16; }

// the LDS of one workgroup for `tile` evaluations; fills the offsets
int lay_out(TrainDesc &d, int tile)
{
    const int KS = d.n_in_fns > 0 ? d.n_in_fns : 1, S = d.H + d.O * d.H + d.O, waves = d.threads / kWave;
    d.lds_stage = up16(d.I * d.HP * 4);
    d.lds_d1 = d.lds_stage + up16((tile + d.T - 1) * d.FP * 4);
    d.lds_stats = d.lds_d1 + up16(tile * d.HP * 4);
    d.lds_red = d.lds_stats + tile * KS * 16;
    d.lds_sel = d.lds_red + up16(waves * 16 + waves * S * 4);
    d.lds_total = d.lds_sel + up16(tile * 4);
    return d.lds_total;
}

template <int HP>
hipError_t launch_gradient(const TrainDesc &d, int groups, const float *columns, int64_t row_stride, const float *params, const float *targets,
                           const float *weights, int64_t n_evals, int tiles_per_row, int n_tiles, double *part, hipStream_t stream)
{
    hipLaunchKernelGGL(train_gradient_kernel<HP>, dim3((unsigned)groups), dim3((unsigned)d.threads), (size_t)d.lds_total, stream, d, columns, row_stride, params, targets,
                       weights, n_evals, tiles_per_row, n_tiles, part);
    return hipGetLastError();
}

}  // namespace

bool train_plan(TrainDesc &d)
{
    if (d.H < 1 || d.H > kTrainMaxHidden || d.O < 1 || d.O > kTrainMaxOut || d.F < 1 || d.T < 1 || d.I != d.F * d.T || d.I > (1 << 16)) return false;
    d.HP = d.H <= 4 ? 4 : d.H <= 8 ? 8 : 16;
    d.FP = d.F | 1;
    // the workgroup: of 256, 320, .. 512 threads the first count that leaves the fewest idle in the passes over the I input positions
    int idle = 1 << 30;
    for (int nt = 256; nt <= 512; nt += kWave) {
        const int w = (d.I + nt - 1) / nt * nt - d.I;
        if (w < idle) {
            idle = w;
            d.threads = nt;
        }
    }
    // the tile: the most evaluations (a multiple of 32, a thread each) whose LDS lets two workgroups share a CU, else one
    d.tile = 0;
    for (int limit : {kLdsComfort, kLdsLimit}) {
        for (int tile = d.threads; tile >= 32 && !d.tile; tile -= 32)
            if (lay_out(d, tile) <= limit) d.tile = tile;
        if (d.tile) break;
    }
    if (!d.tile) return false;
    lay_out(d, d.tile);
    const int64_t per = ((int64_t)train_param_count(d.I, d.H, d.O) + 2) * 8;
    const int64_t fit = ((int64_t)32 << 20) / per;
    d.max_groups = (int)(fit < 64 ? 64 : fit > 1024 ? 1024 : fit);
    return true;
}

// Once a trainer and device, at creation: a workgroup's LDS above 64 KB is allowed for the instantiation the shape takes, so that a
// launch is a launch only.
hipError_t train_prepare(const TrainDesc &d)
{
    if (d.lds_total <= 64 * 1024) return hipSuccess;
    const void *kern = d.HP == 4 ? (const void *)train_gradient_kernel<4> : d.HP == 8 ? (const void *)train_gradient_kernel<8> : (const void *)train_gradient_kernel<16>;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_total);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)train_range_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_total);
}

int train_groups(const TrainDesc &d, int rows, int64_t n_evals)
{
    const int64_t tiles = (int64_t)rows * ((n_evals + d.tile - 1) / d.tile);
    return (int)(tiles < d.max_groups ? tiles : d.max_groups);
}

hipError_t launch_train_targets(const TrainTargetsDesc &d, int64_t n_evals, float *targets, float *weights, hipStream_t stream)
{
    if (n_evals <= 0 || d.rows <= 0) return hipSuccess;
    const dim3 grid((unsigned)((n_evals + kTargetsThreads - 1) / kTargetsThreads), (unsigned)d.rows);
    hipLaunchKernelGGL(train_targets_kernel, grid, dim3(kTargetsThreads), 0, stream, d, n_evals, targets, weights);
    return hipGetLastError();
}

hipError_t launch_train_gradient(const TrainDesc &d, const float *columns, int64_t row_stride, int rows, const float *params, const float *targets,
                                 const float *weights, int64_t n_evals, double *part, hipStream_t stream)
{
    const int groups = train_groups(d, rows, n_evals);
    if (groups <= 0) return hipSuccess;
    const int tiles_per_row = (int)((n_evals + d.tile - 1) / d.tile), n_tiles = rows * tiles_per_row;
    if (d.HP == 4) return launch_gradient<4>(d, groups, columns, row_stride, params, targets, weights, n_evals, tiles_per_row, n_tiles, part, stream);
    if (d.HP == 8) return launch_gradient<8>(d, groups, columns, row_stride, params, targets, weights, n_evals, tiles_per_row, n_tiles, part, stream);
    return launch_gradient<16>(d, groups, columns, row_stride, params, targets, weights, n_evals, tiles_per_row, n_tiles, part, stream);
}

hipError_t launch_train_combine(const TrainDesc &d, int groups, const double *part, double *loss, float *gradient, hipStream_t stream)
{
    const int P = train_param_count(d.I, d.H, d.O);
    hipLaunchKernelGGL(train_combine_kernel, dim3((unsigned)((P + 2 + 255) / 256)), dim3(256), 0, stream, P, groups, part, loss, gradient);
    return hipGetLastError();
}

int train_first_map(const TrainDesc &d)
{
    for (int k = 0; k < d.n_in_fns; k++)
        if (d.in_fns[k].kind == 3) return k;
    return -1;
}

hipError_t launch_train_range(const TrainDesc &d, int at, const float *columns, int64_t row_stride, int rows, const float *weights, int64_t n_evals,
                              double *part, hipStream_t stream)
{
    const int groups = train_groups(d, rows, n_evals);
    if (groups <= 0) return hipSuccess;
    const int tiles_per_row = (int)((n_evals + d.tile - 1) / d.tile), n_tiles = rows * tiles_per_row;
    hipLaunchKernelGGL(train_range_kernel, dim3((unsigned)groups), dim3((unsigned)d.threads), (size_t)d.lds_total, stream, d, at, columns, row_stride, weights, n_evals,
                       tiles_per_row, n_tiles, part);
    return hipGetLastError();
}

hipError_t launch_train_range_combine(const TrainDesc &d, int groups, const double *part, float *range, int64_t *count, hipStream_t stream)
{
    hipLaunchKernelGGL(train_range_combine_kernel, dim3((unsigned)((d.I + 255) / 256)), dim3(256), 0, stream, d.I, train_param_count(d.I, d.H, d.O), groups, part, range,
                       count);
    return hipGetLastError();
}

}  // namespace sd
