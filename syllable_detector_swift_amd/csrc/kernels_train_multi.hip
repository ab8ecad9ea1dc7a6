// kernels_train_multi.hip -- the multi form of the training kernels (syldet_trainer_create_multi of include/syldet.h): a network per
// row.  The kernels are train_kernels.hpp's, the text the plain trainer runs (kernels_train.hip has the notes), instantiated with the
// multi form's arguments:
//   train_gradient_kernel, train_range_kernel   grid (min(the most rows of one network x tiles a row, max_groups), N).  Workgroup (g, n)
//                  reads net_row_begin[n .. n + 1], leaves at once unless g < G_n = min(network n's tiles, max_groups), takes network
//                  n's TrainDesc (its maps, its functions' y) and parameters, and is then workgroup g of G_n of a plain launch over the
//                  network's rows alone: tile tl of the network is tile tl % tiles_per_row of row rows[net_row_begin[n] + tl /
//                  tiles_per_row].  Its partial is n max_groups + g.
//   train_combine_kernel, train_range_combine_kernel   grid.y = N: network n's G_n partials in group order, into its own results.
// The grid is sized by the network with the most rows: in an unbalanced bank most workgroups of the other networks leave at once,
// which costs their dispatch and nothing else.  In a code object of its own, beside the plain trainer's.  gfx950 only.

#include "generic_eval.hpp"
#include "train_kernels.hpp"

namespace sd {

namespace {

// the multi form's grid: (the most workgroups one network gets, N); 0 where no network has a tile
dim3 multi_grid(const TrainDesc &d, const TrainMulti &mu, int64_t n_evals, int *tiles_per_row)
{
    *tiles_per_row = (int)((n_evals + d.tile - 1) / d.tile);
    const int64_t most = (int64_t)mu.max_rows * *tiles_per_row;
    return dim3((unsigned)(most < d.max_groups ? most : d.max_groups), (unsigned)mu.n_nets);
}

template <int HP>
hipError_t launch_gradient_multi(const TrainDesc &d, const TrainMulti &mu, const float *columns, int64_t row_stride, const float *params, const float *targets,
                                 const float *weights, int64_t n_evals, double *part, hipStream_t stream)
{
    int tiles_per_row = 0;
    const dim3 grid = multi_grid(d, mu, n_evals, &tiles_per_row);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    hipLaunchKernelGGL((train_gradient_kernel<HP, TrainMulti>), grid, dim3((unsigned)d.threads), (size_t)d.lds_total, stream, d, columns, row_stride, params, targets, weights,
                       n_evals, tiles_per_row, d.max_groups, part, mu);
    return hipGetLastError();
}

}  // namespace

hipError_t train_prepare_multi(const TrainDesc &d)
{
    if (d.lds_total <= 64 * 1024) return hipSuccess;
    const void *kern = d.HP == 4   ? (const void *)train_gradient_kernel<4, TrainMulti>
                       : d.HP == 8 ? (const void *)train_gradient_kernel<8, TrainMulti>
                                   : (const void *)train_gradient_kernel<16, TrainMulti>;
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_total);
    return e != hipSuccess ? e : hipFuncSetAttribute((const void *)train_range_kernel<TrainMulti>, hipFuncAttributeMaxDynamicSharedMemorySize, d.lds_total);
}

hipError_t launch_train_gradient_multi(const TrainDesc &d, const TrainMulti &mu, const float *columns, int64_t row_stride, const float *params,
                                       const float *targets, const float *weights, int64_t n_evals, double *part, hipStream_t stream)
{
    if (d.HP == 4) return launch_gradient_multi<4>(d, mu, columns, row_stride, params, targets, weights, n_evals, part, stream);
    if (d.HP == 8) return launch_gradient_multi<8>(d, mu, columns, row_stride, params, targets, weights, n_evals, part, stream);
    return launch_gradient_multi<16>(d, mu, columns, row_stride, params, targets, weights, n_evals, part, stream);
}

hipError_t launch_train_combine_multi(const TrainDesc &d, const TrainMulti &mu, int64_t n_evals, const double *part, double *loss, float *gradient,
                                      hipStream_t stream)
{
    if (mu.n_nets <= 0) return hipSuccess;
    const int P = train_param_count(d.I, d.H, d.O), tiles_per_row = (int)((n_evals + d.tile - 1) / d.tile);
    hipLaunchKernelGGL((train_combine_kernel<TrainMulti, int>), dim3((unsigned)((P + 2 + 255) / 256), (unsigned)mu.n_nets), dim3(256), 0, stream, P, d.max_groups, part, loss,
                       gradient, mu, tiles_per_row);
    return hipGetLastError();
}

hipError_t launch_train_range_multi(const TrainDesc &d, const TrainMulti &mu, int at, const float *columns, int64_t row_stride, const float *weights,
                                    int64_t n_evals, double *part, hipStream_t stream)
{
    int tiles_per_row = 0;
    const dim3 grid = multi_grid(d, mu, n_evals, &tiles_per_row);
    if (grid.x == 0 || grid.y == 0) return hipSuccess;
    hipLaunchKernelGGL(train_range_kernel<TrainMulti>, grid, dim3((unsigned)d.threads), (size_t)d.lds_total, stream, d, at, columns, row_stride, weights, n_evals,
                       tiles_per_row, d.max_groups, part, mu);
    return hipGetLastError();
}

hipError_t launch_train_range_combine_multi(const TrainDesc &d, const TrainMulti &mu, int64_t n_evals, const double *part, float *range, int64_t *count,
                                            hipStream_t stream)
{
    if (mu.n_nets <= 0) return hipSuccess;
    const int tiles_per_row = (int)((n_evals + d.tile - 1) / d.tile);
    hipLaunchKernelGGL((train_range_combine_kernel<TrainMulti, int>), dim3((unsigned)((d.I + 255) / 256), (unsigned)mu.n_nets), dim3(256), 0, stream, d.I,
                       train_param_count(d.I, d.H, d.O), d.max_groups, part, range, count, mu, tiles_per_row);
    return hipGetLastError();
}

}  // namespace sd
