// syldet_train_adam.cpp -- the host-only arithmetic of training from the tool (include/syldet.h): the Adam step in the text the
// kernel runs (train_adam.hpp), the input map of a range, and the seeded starting weights.  No device code here.  Built with
// -ffp-contract=off (Makefile), as kernels_train_adam.hip is.

#include <cmath>

#include "syldet_internal.hpp"
#include "train_adam.hpp"

using namespace sd;

extern "C" {

int syldet_train_adam_host(float *params, float *m, float *v, const float *gradient, int64_t n_params, const double *loss, int64_t step, double lr,
                           double beta1, double beta2, double eps, double *mean_loss)
{
    if (n_params < 0 || (n_params > 0 && (!params || !m || !v || !gradient)) || !loss) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    if (const char *why = train_adam_refusal(step, lr, beta1, beta2, eps)) return fail(SYLDET_ERR_INVALID_ARGUMENT, why);
    const TrainAdamStep k = train_adam_consts(step, lr, beta1, beta2, eps);
    const double wsum = loss[1];
    const float s = train_adam_scale(wsum);
    for (int64_t p = 0; p < n_params; p++) train_adam_element(k, wsum > 0.0, s, gradient[p], m + p, v + p, params + p);
    if (mean_loss) *mean_loss = train_adam_mean(loss[0], wsum);
    return SYLDET_OK;
}

int syldet_train_input_map_host(const float *range, int32_t n_inputs, float *x_offsets, float *gains)
{
    if (n_inputs < 0 || (n_inputs > 0 && (!range || !x_offsets || !gains))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    for (int32_t i = 0; i < n_inputs; i++) {
        const float lo = range[i], hi = range[n_inputs + i];
        const float width = hi - lo;
        x_offsets[i] = lo;
        gains[i] = width > 0.0f ? 2.0f / width : 1.0f;
    }
    return SYLDET_OK;
}

int syldet_train_init_host(uint64_t seed, int32_t n_inputs, int32_t n_hidden, int32_t n_outputs, float *theta)
{
    if (n_inputs < 1 || n_hidden < 1 || n_outputs < 1 || !theta) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a count below 1");
    uint64_t state = seed;
    const auto draw = [&state]() {                         // SplitMix64; the top 24 bits as a float in [-1, 1), exact
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (float)(z >> 40) * 0x1p-23f - 1.0f;
    };
    const float w1 = (float)std::sqrt(3.0 / (double)n_inputs), w2 = (float)std::sqrt(3.0 / (double)n_hidden);
    int64_t at = 0;
    for (int64_t k = 0; k < (int64_t)n_hidden * n_inputs; k++) theta[at++] = draw() * w1;
    for (int32_t k = 0; k < n_hidden; k++) theta[at++] = draw() * 0.35f;
    for (int64_t k = 0; k < (int64_t)n_outputs * n_hidden; k++) theta[at++] = draw() * w2;
    for (int32_t k = 0; k < n_outputs; k++) theta[at++] = 0.0f;
    return SYLDET_OK;
}

}  // extern "C"
