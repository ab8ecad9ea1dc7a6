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
// The text of the last four is train_kernels.hpp's, which kernels_train_multi.hip instantiates a second time with the multi form's
// arguments (a network per row, syldet_trainer_create_multi); this file holds the targets kernel, the plain instantiations and the plan.
//
// gfx950 only: wave = 64 lanes.  Plain HIP C++, vector loads and stores, no float atomics.

#include "carve.hpp"
#include "generic_eval.hpp"
#include "train_kernels.hpp"
#include "train_targets.hpp"

namespace sd {

namespace {

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
        const int at = span_at_or_before(d.dets, d.row_begin, row, e);
        has = at >= 0 && e - d.dets[at].first < d.dets[at].units;
        if (has) {
            det = d.dets[at].det;
            own = e - d.dets[at].first;
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

// The kernels are train_kernels.hpp's templates without the multi form's arguments (the multi forms are kernels_train_multi.hip's).
// The table names every instantiation once, for train_prepare, and fixes their order in the code object: instantiations are
// emitted in the order of their first use.
enum PlainKernel { kCombine, kRange, kRangeCombine, kGradient4, kGradient8, kGradient16 };
using GradientFn = void (*)(TrainDesc, const float *, int64_t, const float *, const float *, const float *, int64_t, int, int, double *);
const void *const kPlainKernels[] = {
    (const void *)static_cast<void (*)(int, int, const double *, double *, float *)>(train_combine_kernel<>),
    (const void *)static_cast<void (*)(TrainDesc, int, const float *, int64_t, const float *, int64_t, int, int, double *)>(train_range_kernel<>),
    (const void *)static_cast<void (*)(int, int, int, const double *, float *, int64_t *)>(train_range_combine_kernel<>),
    (const void *)static_cast<GradientFn>(train_gradient_kernel<4>),
    (const void *)static_cast<GradientFn>(train_gradient_kernel<8>),
    (const void *)static_cast<GradientFn>(train_gradient_kernel<16>),
};

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
    hipLaunchKernelGGL(train_gradient_kernel<HP>, dim3((unsigned)groups), dim3((unsigned)d.threads), (size_t)d.lds_total, stream, d, columns, row_stride, params,
                       targets, weights, n_evals, tiles_per_row, n_tiles, part);
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
    const void *kern = kPlainKernels[d.HP == 4 ? kGradient4 : d.HP == 8 ? kGradient8 : kGradient16];
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_total);
    return e != hipSuccess ? e : hipFuncSetAttribute(kPlainKernels[kRange], hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_total);
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
    hipLaunchKernelGGL(train_combine_kernel<>, dim3((unsigned)((P + 2 + 255) / 256)), dim3(256), 0, stream, P, groups, part, loss, gradient);
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
    hipLaunchKernelGGL(train_range_kernel<>, dim3((unsigned)groups), dim3((unsigned)d.threads), (size_t)d.lds_total, stream, d, at, columns, row_stride, weights,
                       n_evals, tiles_per_row, n_tiles, part);
    return hipGetLastError();
}

hipError_t launch_train_range_combine(const TrainDesc &d, int groups, const double *part, float *range, int64_t *count, hipStream_t stream)
{
    hipLaunchKernelGGL(train_range_combine_kernel<>, dim3((unsigned)((d.I + 255) / 256)), dim3(256), 0, stream, d.I, train_param_count(d.I, d.H, d.O), groups, part,
                       range, count);
    return hipGetLastError();
}

}  // namespace sd
