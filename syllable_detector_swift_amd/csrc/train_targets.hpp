// train_targets.hpp -- the trainer's targets (include/syldet.h, "training"): which outputs' target is 1 at one evaluation of one
// detector, and the class weight that goes with it.  One text for the device (train_targets_kernel, kernels_train.hip), the host
// (syldet_train_targets_host, syldet_train.cpp) and a stand-alone test (tests/cpp/train_targets_test.cpp).  int64 arithmetic and
// two float constants; nothing is computed in floating point.
//   train_target_mask    (idx, the detector's sorted labels and their outputs, half width) -> bit o set iff some label j with
//                        label_output[j] == o has |idx - t_j| <= half_width
//   train_target_write   the mask as O floats of 1.0 / 0.0 and the weight: weight_positive where any bit is set, else weight_negative
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_TRAIN_FN __host__ __device__ __forceinline__
#else
#define SD_TRAIN_FN inline
#endif

namespace sd {

constexpr int kTrainMaxHidden = 16;                          // H <= 16, O <= 4: the fold kernel's envelope
constexpr int kTrainMaxOut = 4;
constexpr int64_t kTrainMaxHalfWidth = (int64_t)1 << 40;     // 0 <= half_width <= 2^40
constexpr int64_t kTrainIndexLimit = (int64_t)1 << 62;       // |idx| < 2^62: idx +- half_width cannot overflow

// labels: n sorted sample numbers (any int64; they may repeat, overlap, lie before 0 or behind the detector's end); label_output:
// each label's output (NULL: all 0).
SD_TRAIN_FN uint32_t train_target_mask(int64_t idx, const int64_t *labels, const int32_t *label_output, int64_t n, int64_t half_width)
{
    const int64_t a = idx - half_width, b = idx + half_width;
    int64_t lo = 0, hi = n;                                  // the first label >= a
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (labels[mid] < a) lo = mid + 1;
        else hi = mid;
    }
    uint32_t mask = 0;
    for (int64_t j = lo; j < n && labels[j] <= b; j++) mask |= 1u << (label_output ? label_output[j] : 0);
    return mask;
}

SD_TRAIN_FN void train_target_write(uint32_t mask, int n_out, float weight_positive, float weight_negative, float *target, float *weight)
{
    for (int o = 0; o < n_out; o++) target[o] = (mask >> o) & 1u ? 1.0f : 0.0f;
    *weight = mask ? weight_positive : weight_negative;
}

}  // namespace sd
