// kernels_train_adam.hip -- the optimiser's step on the device (syldet_train_adam_device of include/syldet.h).
//
//   train_adam_kernel   A thread a parameter: train_adam.hpp, the text the host runs.  The loss and the weight sum are read where
//                  the combine kernel left them, so nothing comes back to the host between the gradient and the step.  Thread 0
//                  also writes the mean loss L / Wsum.
//   train_adam_multi_kernel   The same over [N][P] (syldet_trainer_create_multi): an element's network is p / P, and the loss, the
//                  weight sum and the mean loss are that network's.
//
// Built with -ffp-contract=off (Makefile): a product and a sum stay two roundings, as on the host.  gfx950 only.

#include "kernels.hpp"
#include "train_adam.hpp"

namespace sd {

namespace {

constexpr int kAdamThreads = 256;

__global__ void __launch_bounds__(kAdamThreads)
train_adam_kernel(TrainAdamStep k, int P, const double *__restrict__ loss, const float *__restrict__ gradient, float *__restrict__ m, float *__restrict__ v,
                  float *__restrict__ params, double *__restrict__ mean_loss)
{
    const int p = (int)blockIdx.x * kAdamThreads + (int)threadIdx.x;
    if (p >= P) return;
    const double wsum = loss[1];
    train_adam_element(k, wsum > 0.0, train_adam_scale(wsum), gradient[p], m + p, v + p, params + p);
    if (p == 0 && mean_loss) *mean_loss = train_adam_mean(loss[0], wsum);
}

// The multi form: params, gradient, m and v are [N][P], loss [N][2], mean_loss [N]; an element's network is p / P, and 1 / Wsum is
// that network's.  Element for element the text above.
__global__ void __launch_bounds__(kAdamThreads)
train_adam_multi_kernel(TrainAdamStep k, int P, int64_t total, const double *__restrict__ loss, const float *__restrict__ gradient, float *__restrict__ m,
                        float *__restrict__ v, float *__restrict__ params, double *__restrict__ mean_loss)
{
    const int64_t p = (int64_t)blockIdx.x * kAdamThreads + (int64_t)threadIdx.x;
    if (p >= total) return;
    const int64_t net = p / P;
    const double wsum = loss[2 * net + 1];
    train_adam_element(k, wsum > 0.0, train_adam_scale(wsum), gradient[p], m + p, v + p, params + p);
    if (p == net * P && mean_loss) mean_loss[net] = train_adam_mean(loss[2 * net], wsum);
}

}  // namespace

hipError_t launch_train_adam_multi(const TrainAdamStep &k, int P, int n_nets, const double *loss, const float *gradient, float *m, float *v, float *params,
                                   double *mean_loss, hipStream_t stream)
{
    const int64_t total = (int64_t)P * n_nets;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(train_adam_multi_kernel, dim3((unsigned)((total + kAdamThreads - 1) / kAdamThreads)), dim3(kAdamThreads), 0, stream, k, P, total, loss, gradient,
                       m, v, params, mean_loss);
    return hipGetLastError();
}

hipError_t launch_train_adam(const TrainAdamStep &k, int P, const double *loss, const float *gradient, float *m, float *v, float *params, double *mean_loss,
                             hipStream_t stream)
{
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(train_adam_kernel, dim3((unsigned)((P + kAdamThreads - 1) / kAdamThreads)), dim3(kAdamThreads), 0, stream, k, P, loss, gradient, m, v, params,
                       mean_loss);
    return hipGetLastError();
}

}  // namespace sd
