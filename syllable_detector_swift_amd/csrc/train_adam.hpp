// train_adam.hpp -- the optimiser's step (include/syldet.h, "training from the tool"): Adam on one element, in fp32.  One text for
// the device (train_adam_kernel, kernels_train_adam.hip), the host (syldet_train_adam_host, syldet_train_adam.cpp) and a stand-alone
// test (tests/cpp/train_adam_test.cpp); all three are built with -ffp-contract=off and no fast-math flag, so every operation below
// rounds to fp32 on its own and the three agree to the bit.
//   train_adam_refusal   the arguments a step does not take, as a message
//   train_adam_consts    (step t >= 1, lr, beta1, beta2, eps in double) -> the step's fp32 constants; pow and sqrt in double, on the host
//   train_adam_scale     Wsum -> s = 1 / Wsum as fp32, or 0 where Wsum is not above 0
//   train_adam_mean      (L, Wsum) -> L / Wsum, or 0 where Wsum is not above 0
//   train_adam_element   one parameter: g = grad s; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g g; p = p - c1 (m / (sqrt(v) c2 + eps)).
//                        At step 1 the old m and v are not read and count as 0.  Where Wsum is not above 0 p is left as it is.
#pragma once

#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_ADAM_FN __host__ __device__ __forceinline__
#else
#define SD_ADAM_FN inline
#endif

namespace sd {

struct TrainAdamStep {
    float b1, omb1, b2, omb2;                // beta1, 1 - beta1, beta2, 1 - beta2 (each difference in double, rounded once)
    float c1, c2, eps;                       // lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), eps
    int first;                               // t == 1: the moments start from 0
};

// what a step refuses (nullptr: nothing): the one check of the device call, the fit and the host function
inline const char *train_adam_refusal(int64_t t, double lr, double beta1, double beta2, double eps)
{
    if (t < 1 || t > ((int64_t)1 << 31)) return "the step number must be in [1, 2^31]";
    if (!std::isfinite(lr) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !std::isfinite(eps))
        return "lr must be finite, beta1 and beta2 in [0, 1), eps finite and 0 or more";
    return nullptr;
}

inline TrainAdamStep train_adam_consts(int64_t t, double lr, double beta1, double beta2, double eps)
{
    TrainAdamStep k;
    k.b1 = (float)beta1;
    k.omb1 = (float)(1.0 - beta1);
    k.b2 = (float)beta2;
    k.omb2 = (float)(1.0 - beta2);
    k.c1 = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    k.c2 = (float)(1.0 / std::sqrt(1.0 - std::pow(beta2, (double)t)));
    k.eps = (float)eps;
    k.first = t == 1 ? 1 : 0;
    return k;
}

SD_ADAM_FN float train_adam_scale(double wsum) { return wsum > 0.0 ? (float)(1.0 / wsum) : 0.0f; }

SD_ADAM_FN double train_adam_mean(double loss, double wsum) { return wsum > 0.0 ? loss / wsum : 0.0; }

SD_ADAM_FN void train_adam_element(const TrainAdamStep &k, bool moves, float s, float grad, float *m, float *v, float *p)
{
    const float g = grad * s;
    const float m0 = k.first ? 0.0f : *m, v0 = k.first ? 0.0f : *v;
    const float gg = g * g;
    const float m1 = k.b1 * m0 + k.omb1 * g;
    const float v1 = k.b2 * v0 + k.omb2 * gg;
    *m = m1;
    *v = v1;
    if (moves) {
        const float root = sqrtf(v1);
        const float den = root * k.c2 + k.eps;
        const float q = m1 / den;
        *p = *p - k.c1 * q;
    }
}

}  // namespace sd
