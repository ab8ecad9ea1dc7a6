// detector_spans.hpp -- the one detector table of the handles that sit on a bank and, optionally, on a packed-recordings plan
// (the scorer, the aligner, the trainer, the matchers): detector d's row, first unit and unit count.  On a plain bank detector d is
// row d, all of it, and there is no table; on a packed plan it is a stretch of a row, a DetSpan.
//   span_of, span_row_units     a plan's slot, and a row's length, in a handle's unit (samples, frames or evaluations)
//   spans_first_beyond          the bounds rule: the first span that leaves its row
//   spans_by_row                the table a kernel searches: sorted by (row, first, units), with row_begin
//   span_at_or_before           that search, one text for the kernels (kernels_train.hip, kernels_match.hip) and the host
// The host part needs no HIP header: a plain host program holds all of it (tests/cpp/detector_spans_test.cpp).  Not installed.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "syldet_internal.hpp"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_SPAN_FN __host__ __device__ __forceinline__
#else
#define SD_SPAN_FN inline
#endif

namespace sd {

// A detector of a packed plan: its unit 0 is unit `first` of row `row`, and it has `units` units.  det: the recording, its index
// in the caller's order (what a by_row table gives back).
struct DetSpan {
    int64_t first, units;
    int32_t det, row;
};
static_assert(sizeof(DetSpan) == 24, "the kernels read the table in 24-byte entries");

enum SpanUnit { kSpanSamples, kSpanFrames, kSpanEvals };

// a slot of the plan in a unit: frames are whole frames of the recording's own samples from its first evaluation's frame on
inline DetSpan span_of(const syldet_slot_t &p, int32_t det, const BankInfo &b, SpanUnit unit)
{
    if (unit == kSpanSamples) return DetSpan{p.offset, p.n_samples, det, p.row};
    if (unit == kSpanEvals) return DetSpan{p.first_eval, p.n_evals, det, p.row};
    return DetSpan{p.first_eval, std::max<int64_t>(0, count_frames(b.geom, b.window_length, p.n_samples)), det, p.row};
}

// ... and the packed rows' length in it (row_samples and row_evals: syldet_recordings_shape's)
inline int64_t span_row_units(const BankInfo &b, SpanUnit unit, int64_t row_samples, int64_t row_evals)
{
    if (unit == kSpanSamples) return row_samples;
    if (unit == kSpanEvals) return row_evals;
    return std::max<int64_t>(0, count_frames(b.geom, b.window_length, row_samples));
}

// The bounds rule: every row is in [0, rows), and a span that has units lies in [0, row_units) of its row (one without units
// may stand anywhere: nothing of it is read).  The index of the first span that breaks it, -1 for none.
inline int64_t spans_first_beyond(const DetSpan *spans, int64_t n, int rows, int64_t row_units)
{
    for (int64_t k = 0; k < n; k++) {
        const DetSpan &e = spans[k];
        if (e.row < 0 || e.row >= rows || (e.units > 0 && (e.first < 0 || e.first + e.units > row_units))) return k;
    }
    return -1;
}

// The table the kernels search: the spans by (row, first, units), row c's are [row_begin[c], row_begin[c + 1]).  A recording
// without units sorts in front of one that starts at the same unit, so that the last span at or before a unit is the one that
// holds it.  The spans have passed spans_first_beyond.
inline void spans_by_row(const std::vector<DetSpan> &spans, int rows, std::vector<DetSpan> *by_row, std::vector<int32_t> *row_begin)
{
    *by_row = spans;
    std::stable_sort(by_row->begin(), by_row->end(), [](const DetSpan &x, const DetSpan &y) {
        if (x.row != y.row) return x.row < y.row;
        return x.first != y.first ? x.first < y.first : x.units < y.units;
    });
    row_begin->assign((size_t)rows + 1, 0);
    for (const DetSpan &e : *by_row) (*row_begin)[(size_t)e.row + 1]++;
    for (int c = 0; c < rows; c++) (*row_begin)[(size_t)c + 1] += (*row_begin)[(size_t)c];
}

// The last entry of row `row` in a by_row table that starts at or before unit q: its index, or -1 where the row has none.
// Whether it still holds q, or a window from q on, is the caller's to ask of its units.
SD_SPAN_FN int span_at_or_before(const DetSpan *by_row, const int32_t *row_begin, int row, int64_t q)
{
    int lo = row_begin[row], hi = row_begin[row + 1];
    const int begin = lo;
    while (lo < hi) {                                        // the first entry that starts behind q
        const int mid = (lo + hi) >> 1;
        if (by_row[mid].first <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo > begin ? lo - 1 : -1;
}

}  // namespace sd
