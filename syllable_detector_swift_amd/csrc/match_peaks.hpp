// match_peaks.hpp -- template matching (include/syldet.h, "template matching"): which positions of one detector's scores are
// MATCHES, and the sample number of a match.  One text for the device (match_peaks_kernel, kernels_match.hip), the host
// (syldet_match_peaks_host, syldet_match.cpp) and a stand-alone test (tests/cpp/match_peaks_test.cpp).  A score enters as its KEY,
// an unsigned integer in the order of the floats; everything behind the key is integer arithmetic.
//   match_key         fp32 score -> key: 0 for a NaN, else increasing with the score (-0.0 and +0.0 share a key)
//   match_level       the largest k with 2^k <= S (S >= 1): windows of S positions are two windows of 2^k
//   match_left / match_right   the largest key in [p - S, p) / (p, p + S] from the table m of maxima over [i, i + 2^k)
//   match_rule        key, the two maxima, the threshold's key -> is the position a match
//   match_event       origin + (p + anchor) hop
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_MATCH_FN __host__ __device__ __forceinline__
#else
#define SD_MATCH_FN inline
#endif

namespace sd {

constexpr int kMatchMaxTemplate = 32768;                     // n bins <= 2^15 elements
constexpr int kMatchMaxSeparation = 4096;                    // 0 <= S <= 4096 positions

// NaN -> 0; any other score -> a key in [0x007fffff, 0xff800000] that orders as the scores do (-inf lowest, +inf highest).  A NaN's
// key is below every score's: a NaN neither matches nor suppresses.
SD_MATCH_FN uint32_t match_key(float s)
{
    if (s != s) return 0u;
    s = s + 0.0f;                                            // -0.0 -> +0.0: the two compare equal, so they share a key
    uint32_t u;
    __builtin_memcpy(&u, &s, sizeof(u));
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

SD_MATCH_FN int match_level(int S)                           // S >= 1
{
    int k = 0;
    while ((2 << k) <= S) k++;
    return k;
}

// m[i] = the largest key of positions [i - base, i - base + 2^k) of the detector (positions outside it hold key 0); m covers
// [p - S, p + S] of every p asked for.  S == 0: no neighbour, 0.
SD_MATCH_FN uint32_t match_left(const uint32_t *m, int64_t i, int S, int k)      // i = p + base
{
    if (S == 0) return 0u;
    const uint32_t a = m[i - S], b = m[i - ((int64_t)1 << k)];
    return a > b ? a : b;
}
SD_MATCH_FN uint32_t match_right(const uint32_t *m, int64_t i, int S, int k)
{
    if (S == 0) return 0u;
    const uint32_t a = m[i + 1], b = m[i + S + 1 - ((int64_t)1 << k)];
    return a > b ? a : b;
}

// the score is not NaN, is at least the threshold, is above everything S before it and not below anything S behind it: the
// earliest position of a tie wins
SD_MATCH_FN bool match_rule(uint32_t key, uint32_t left, uint32_t right, uint32_t threshold_key)
{
    return key != 0u && key >= threshold_key && left < key && right <= key;
}

SD_MATCH_FN int64_t match_event(int64_t origin, int64_t hop, int64_t p, int64_t anchor) { return origin + (p + anchor) * hop; }

}  // namespace sd
