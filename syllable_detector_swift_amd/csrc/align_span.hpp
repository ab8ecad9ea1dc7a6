// align_span.hpp -- event-aligned windows (include/syldet.h, "event-aligned windows"): what one event selects of one detector's
// units.  One text for the device (align_windows_kernel, kernels_align.hip), the host (syldet_align_host, syldet_align.cpp) and a
// stand-alone test (tests/cpp/align_span_test.cpp).  int64 arithmetic with a floor division; no float is involved.
//   align_floor_div   floor(a / b) for b >= 1, also for a < 0 (C++ division truncates)
//   align_span        (s, origin, step, before, after, U) -> the window's present units: where they begin in the window, how many
//                     they are, and which unit of the detector is the first of them
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_ALIGN_FN __host__ __device__ __forceinline__
#else
#define SD_ALIGN_FN inline
#endif

namespace sd {

// sources (SYLDET_ALIGN_* of include/syldet.h)
enum { kAlignColumns = 0, kAlignOutputs = 1, kAlignSamples = 2 };

constexpr int64_t kAlignEventLimit = (int64_t)1 << 62;       // |s| < 2^62
constexpr int64_t kAlignMaxWindow = (int64_t)1 << 20;        // n * width <= 2^20 elements

// A window's present part.  Window unit j (0 <= j < before + after + 1) is the detector's unit u0 - before + j; the present ones are
// j in [first, first + count), and window unit `first` is the detector's unit `unit`: 0 <= unit and unit + count <= U.  count == 0:
// nothing of the window is present (first and unit are 0).
struct AlignSpan {
    int64_t first, count, unit;
};

SD_ALIGN_FN int64_t align_floor_div(int64_t a, int64_t b)    // b >= 1
{
    const int64_t q = a / b;
    return q * b > a ? q - 1 : q;                            // (only a negative a with a remainder: the truncation went up)
}

// origin and step: the source's anchor rule u0 = floor((s - origin) / step), 0 <= origin < 2^32, 1 <= step < 2^31; 0 <= before, after
// <= 2^20; 0 <= U < 2^62.  An s outside (-2^62, 2^62) -- not an event, by the convention -- is taken as the nearest one inside, so
// that nothing here can overflow whatever an event table holds.
SD_ALIGN_FN AlignSpan align_span(int64_t s, int64_t origin, int64_t step, int64_t before, int64_t after, int64_t U)
{
    s = s < -(kAlignEventLimit - 1) ? -(kAlignEventLimit - 1) : s > kAlignEventLimit - 1 ? kAlignEventLimit - 1 : s;
    const int64_t u0 = align_floor_div(s - origin, step);
    const int64_t lo = u0 - before, hi = u0 + after;         // the window's units, both ends included
    const int64_t a = lo > 0 ? lo : 0, b = hi < U - 1 ? hi : U - 1;
    AlignSpan sp;
    if (b < a) {
        sp.first = sp.count = sp.unit = 0;
        return sp;
    }
    sp.first = a - lo;
    sp.count = b - a + 1;
    sp.unit = a;
    return sp;
}

}  // namespace sd
