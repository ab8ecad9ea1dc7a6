// kernels_train_adam.hip -- the optimiser's step on the device (syldet_train_adam_device of include/syldet.h).
//
//   train_adam_kernel   A thread a parameter: train_adam.hpp, the text the host runs.  The loss and the weight sum are read where
//                  the combine kernel left them, so nothing comes back to the host between the gradient and the step.  Thread 0
//                  also writes the mean loss L / Wsum.
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

}  // namespace

hipError_t launch_train_adam(const TrainAdamStep &k, int P, const double *loss, const float *gradient, float *m, float *v, float *params, double *mean_loss,
                             hipStream_t stream)
{
    if (P <= 0) return hipSuccess;
    hipLaunchKernelGGL(train_adam_kernel, dim3((unsigned)((P + kAdamThreads - 1) / kAdamThreads)), dim3(kAdamThreads), 0, stream, k, P, loss, gradient, m, v, params,
                       mean_loss);
    return hipGetLastError();
}

}  // namespace sd
