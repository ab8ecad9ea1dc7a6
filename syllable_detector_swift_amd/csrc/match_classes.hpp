// match_classes.hpp -- template matching, a bank of templates (include/syldet.h, "template matching: a bank of templates"): the
// score of a CLASS at a position is the greatest of its templates' scores there, and `which` the lowest template that attains it.
// One text for the device (the match_bank_scores kernels, kernels_match.hip), the host (syldet_match_classes_host,
// syldet_match.cpp) and a stand-alone test (tests/cpp/match_classes_test.cpp).  Comparisons of fp32 values only: no arithmetic, so
// the class score has the bits of one of its templates' scores.
//   match_class_begin   the running value before the first template: NaN, which -1
//   match_class_take    template k's score s, taken in ascending k: it replaces the running value only where it is greater (or
//                       where there is none yet); a NaN is never taken, so a position that is NaN for every template stays NaN, -1
//   match_classes       [K][n_positions] template scores -> [C][n_positions] class scores and which (may be NULL)
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_MATCH_CLASS_FN __host__ __device__ __forceinline__
#else
#define SD_MATCH_CLASS_FN inline
#endif

namespace sd {

constexpr int kMatchMaxTemplates = 64;                       // 1 <= K <= 64 templates a bank
constexpr int kMatchMaxClasses = 16;                         // 1 <= C <= 16 classes

SD_MATCH_CLASS_FN void match_class_begin(float &running, int32_t &which)
{
    const uint32_t nan = 0x7fc00000u;
    __builtin_memcpy(&running, &nan, sizeof(nan));
    which = -1;
}

SD_MATCH_CLASS_FN void match_class_take(float s, int32_t k, float &running, int32_t &which)
{
    if (which < 0 ? s == s : s > running) {
        running = s;
        which = k;
    }
}

// every class's plane from the templates' planes; every element of class_scores (and of which, if given) written exactly once.  A
// class without a template is all NaN, -1 (the callers refuse such a table).
SD_MATCH_CLASS_FN void match_classes(const float *template_scores, int64_t n_positions, int32_t n_templates, const int32_t *template_class,
                                     int32_t n_classes, float *class_scores, int32_t *which)
{
    for (int32_t c = 0; c < n_classes; c++)
        for (int64_t p = 0; p < n_positions; p++) {
            float running;
            int32_t w;
            match_class_begin(running, w);
            for (int32_t k = 0; k < n_templates; k++)
                if ((template_class ? template_class[k] : k) == c) match_class_take(template_scores[(int64_t)k * n_positions + p], k, running, w);
            class_scores[(int64_t)c * n_positions + p] = running;
            if (which) which[(int64_t)c * n_positions + p] = w;
        }
}

}  // namespace sd
