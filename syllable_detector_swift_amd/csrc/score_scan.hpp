// score_scan.hpp -- threshold calibration (include/syldet.h, "threshold calibration"): what one threshold does with one evaluation
// that the scan visits.  One text for the device (score_kernel, kernels_score.hip: a lane is a threshold) and the host
// (syldet_score_host, syldet_score.cpp; tests/cpp/score_scan_test.cpp: one threshold after another).
//   score_cursor   the label whose window [t_j - m, t_j + m] may hold sample idx: depends on idx alone (not on the threshold), so
//                  on the device it is the wave's and lives in scalar registers
//   score_step     the debounce rule of TrackDetector.swift:65-100 and the class of the detection it emits, predicated
#pragma once

#include <cmath>
#include <cstdint>
#include <limits>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_SCORE_FN __host__ __device__ __forceinline__
#else
#define SD_SCORE_FN inline
#endif

namespace sd {

// columns of a table row (SYLDET_SCORE_* of include/syldet.h)
enum { kScoreDetections = 0, kScoreHits = 1, kScoreFalsePositives = 2, kScoreRepeats = 3, kScoreSumOffset = 4, kScoreSumOffsetSquared = 5,
       kScoreColumns = 6 };

// one threshold's state on one detector
struct ScoreLane {
    int64_t until = -1;                  // debounceUntil :30
    int64_t n[kScoreColumns] = {0, 0, 0, 0, 0, 0};
    bool hit = false;                    // has this threshold hit the cursor's label already?
};

// The smallest float >= theta (+inf beyond FLT_MAX): Double(v) >= theta exactly where v >= that float, because float -> double
// is exact.  theta is not NaN.
inline float score_threshold_f32(double theta)
{
    float f = (float)theta;
    if ((double)f < theta) f = std::nextafterf(f, std::numeric_limits<float>::infinity());
    return f;
}

// The cursor: j, and t = labels[j] while j < n (so that a visit that does not move it reads no memory).
struct ScoreCursor {
    int64_t j = 0, t = 0;
};

SD_SCORE_FN ScoreCursor score_cursor_start(const int64_t *__restrict__ labels, int64_t n)
{
    ScoreCursor c;
    if (n > 0) c.t = labels[0];
    return c;
}

// Moves the cursor to the first label whose window does not end before idx (t_j + m >= idx; j == n: none left) and says whether
// it moved.  The labels are sorted and idx only grows, so the cursor never goes back.  idx - m cannot overflow (|idx| < 2^62,
// m <= 2^20).
SD_SCORE_FN bool score_cursor(const int64_t *__restrict__ labels, int64_t n, int64_t m, int64_t idx, ScoreCursor &c)
{
    bool moved = false;
    while (c.j < n && c.t < idx - m) {
        c.j++;
        moved = true;
        if (c.j < n) c.t = labels[c.j];
    }
    return moved;
}

// One visited evaluation at sample idx for one threshold.  flag: the output reaches this threshold; moved: the cursor left its
// label at this evaluation (the hit bit belongs to the label, not the threshold); in_window / offset: idx lies in the cursor's
// window, idx - t_j (0 outside).  No branch: every update is a select or an addition of 0 / 1.
SD_SCORE_FN void score_step(ScoreLane &s, bool flag, int64_t idx, int64_t debounce_frames, bool moved, bool in_window, int64_t offset)
{
    const bool emit = flag && s.until < idx;                             // hasDetection && debounceUntil < curOutput :80
    const bool had = s.hit && !moved;
    const bool hit = emit && in_window && !had;
    const bool repeat = emit && in_window && had;
    const bool stray = emit && !in_window;
    s.until = emit ? idx + debounce_frames : s.until;                    // :99
    s.hit = had || hit;
    s.n[kScoreDetections] += emit ? 1 : 0;
    s.n[kScoreHits] += hit ? 1 : 0;
    s.n[kScoreFalsePositives] += stray ? 1 : 0;
    s.n[kScoreRepeats] += repeat ? 1 : 0;
    s.n[kScoreSumOffset] += hit ? offset : 0;
    s.n[kScoreSumOffsetSquared] += hit ? offset * offset : 0;
}

// ... and the two together: one evaluation at sample idx that the scan visits, for the threshold of s (flag: reached).  The
// cursor is the wave's (or the host's): every lane calls this with the same c.
SD_SCORE_FN void score_visit(ScoreLane &s, bool flag, int64_t idx, int64_t debounce_frames, const int64_t *__restrict__ labels, int64_t n, int64_t m,
                             ScoreCursor &c)
{
    const bool moved = score_cursor(labels, n, m, idx, c);
    const bool in_window = c.j < n && c.t <= idx + m;                    // (t >= idx - m: the cursor's own condition)
    score_step(s, flag, idx, debounce_frames, moved, in_window, in_window ? idx - c.t : 0);
}

}  // namespace sd
