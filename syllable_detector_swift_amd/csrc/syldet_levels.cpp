// syldet_levels.cpp -- the host side of the level meters: the library's sum of squares (what vDSP_svesq is to
// Processor.swift:111-113, with the summation order fixed) for the streaming appends, and the count of readings.
//
// Compiled with -ffp-contract=off (see the Makefile): every square and every addition rounds to fp32 on its own.

#include "syldet_internal.hpp"

namespace sd {

namespace {

inline float sample_of(float x) { return x; }
inline float sample_of(int16_t x) { return (float)x * (1.0f / 32768.0f); }   // exact

// The balanced binary tree over next_pow2(n) slots, in index order, slots past n holding +0: a binary counter of finished
// subtrees (level l holds the sum of 2^l squares when bit l of the count is set).  What is left at the end is summed from the
// lowest level up: the missing right halves are +0, and s + (+0) == s (a square is never -0).
template <class T>
float tree(const T *x, int64_t n, int64_t step)
{
    float level[64];
    for (int64_t i = 0; i < n; i++) {
        const float v = sample_of(x[i * step]);
        float s = v * v;
        int l = 0;
        for (int64_t bits = i; bits & 1; bits >>= 1) s = level[l++] + s;
        level[l] = s;
    }
    float s = 0.0f;
    bool any = false;
    for (int l = 0; l < 63; l++)
        if ((n >> l) & 1) {
            s = any ? level[l] + s : level[l];
            any = true;
        }
    return s;
}

}  // namespace

float sum_squares_tree(const float *x, int64_t n, int64_t step) { return tree(x, n, step); }
float sum_squares_tree(const int16_t *x, int64_t n, int64_t step) { return tree(x, n, step); }

}  // namespace sd

extern "C" {

float syldet_sum_squares(const float *x, int64_t n)
{
    if (!x || n <= 0) return 0.0f;
    return sd::sum_squares_tree(x, n, 1);
}

int64_t syldet_levels_count(int64_t n_samples, int32_t buffer_length, int64_t buffers_per_reading)
{
    if (n_samples < 0 || !sd::levels_buffer_ok(buffer_length) || buffers_per_reading < 1) return -1;
    const int64_t B = n_samples / buffer_length + (n_samples % buffer_length != 0);
    return B / buffers_per_reading + (B % buffers_per_reading != 0);
}

}  // extern "C"
