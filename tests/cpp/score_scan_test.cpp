// The per-threshold step of threshold calibration (csrc/score_scan.hpp, what score_kernel's lanes and syldet_score_host run) on
// its own, over hand-worked cases.  Built with -fsanitize=address,undefined by tests/test_score_host.py; every array is exactly
// as long as what is read of it.
#include <cstdio>
#include <limits>
#include <vector>

#include "score_scan.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

struct Row {
    int64_t n[6];
};

// one threshold over one detector, as syldet_score_host walks it
static Row scan(const std::vector<float> &values, double theta, const std::vector<int64_t> &labels, int64_t m, int64_t first_index, int64_t hop,
                int64_t debounce_frames)
{
    const float thr = sd::score_threshold_f32(theta);
    sd::ScoreLane s;
    const int64_t n = (int64_t)labels.size();
    sd::ScoreCursor c = sd::score_cursor_start(labels.data(), n);
    for (size_t e = 0; e < values.size(); e++) {
        if (!(values[e] >= thr)) continue;
        sd::score_visit(s, true, first_index + (int64_t)e * hop, debounce_frames, labels.data(), n, m, c);
    }
    Row r;
    for (int c = 0; c < 6; c++) r.n[c] = s.n[c];
    return r;
}

// ... and as a lane of the kernel walks it: every evaluation that reaches `least` is visited, flag or not
static Row scan_visiting(const std::vector<float> &values, double theta, double least, const std::vector<int64_t> &labels, int64_t m,
                         int64_t first_index, int64_t hop, int64_t debounce_frames)
{
    const float thr = sd::score_threshold_f32(theta), lo = sd::score_threshold_f32(least);
    sd::ScoreLane s;
    const int64_t n = (int64_t)labels.size();
    sd::ScoreCursor c = sd::score_cursor_start(labels.data(), n);
    for (size_t e = 0; e < values.size(); e++) {
        if (!(values[e] >= lo)) continue;
        sd::score_visit(s, values[e] >= thr, first_index + (int64_t)e * hop, debounce_frames, labels.data(), n, m, c);
    }
    Row r;
    for (int c = 0; c < 6; c++) r.n[c] = s.n[c];
    return r;
}

static bool is(const Row &r, int64_t det, int64_t hits, int64_t fp, int64_t rep, int64_t s1, int64_t s2)
{
    return r.n[0] == det && r.n[1] == hits && r.n[2] == fp && r.n[3] == rep && r.n[4] == s1 && r.n[5] == s2;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // first_index 100, hop 10: evaluation e is sample 100 + 10 e
    //                         e:  0     1     2     3     4     5     6     7     8     9
    const std::vector<float> v = {0.1f, 0.9f, 0.9f, 0.1f, 0.6f, 0.1f, 0.1f, 0.9f, 0.1f, 0.95f};
    const std::vector<int64_t> lab = {112, 171};
    // theta 0.5, no debounce, tolerance 5: detections at 110 (hit, -2), 120 (fp), 140 (fp), 170 (hit, -1), 190 (fp)
    CHECK(is(scan(v, 0.5, lab, 5, 100, 10, 0), 5, 2, 3, 0, -3, 5));
    // tolerance 8: 120 is inside [104, 120] too: a repeat of label 0
    CHECK(is(scan(v, 0.5, lab, 8, 100, 10, 0), 5, 2, 2, 1, -3, 5));
    // debounce 10 frames: 110 fires, until = 120 swallows 120 (not 120 < 120); 140, 170, 190 fire
    CHECK(is(scan(v, 0.5, lab, 8, 100, 10, 10), 4, 2, 2, 0, -3, 5));
    // debounce 9: until = 119 < 120: as without
    CHECK(is(scan(v, 0.5, lab, 8, 100, 10, 9), 5, 2, 2, 1, -3, 5));
    // theta 0.7 leaves out 140
    CHECK(is(scan(v, 0.7, lab, 5, 100, 10, 0), 4, 2, 2, 0, -3, 5));
    // a low threshold fires early and the debounce swallows the real crossing: theta 0.05 with 35 frames fires at 100 (fp),
    // 140 (fp), 180 (fp): no hit at all, where theta 0.5 hits both labels (110 and 170; 120, 140 and 190 are swallowed)
    CHECK(is(scan(v, 0.05, lab, 5, 100, 10, 35), 3, 0, 3, 0, 0, 0));
    CHECK(is(scan(v, 0.5, lab, 5, 100, 10, 35), 2, 2, 0, 0, -3, 5));
    // the lane's walk (visits without a flag move the cursor and nothing else) gives the host's rows
    for (double theta : {0.05, 0.5, 0.7, 0.92, 2.0})
        for (int64_t deb : {0, 9, 10, 35})
            for (int64_t m : {0, 5, 8}) {
                const Row a = scan(v, theta, lab, m, 100, 10, deb), b = scan_visiting(v, theta, 0.05, lab, m, 100, 10, deb);
                CHECK(is(b, a.n[0], a.n[1], a.n[2], a.n[3], a.n[4], a.n[5]));
                CHECK(a.n[0] == a.n[1] + a.n[2] + a.n[3]);
            }
    // tolerance 0: only the label's own sample hits
    CHECK(is(scan(v, 0.5, {110, 171}, 0, 100, 10, 0), 5, 1, 4, 0, 0, 0));
    // no labels, no evaluations
    CHECK(is(scan(v, 0.5, {}, 5, 100, 10, 0), 5, 0, 5, 0, 0, 0));
    CHECK(is(scan({}, 0.5, lab, 5, 100, 10, 0), 0, 0, 0, 0, 0, 0));
    // labels before sample 0 and behind the end are misses, not errors; a negative label's window may still hold sample 100
    CHECK(is(scan(v, 0.5, {-500, 112, 100000}, 5, 100, 10, 0), 5, 1, 4, 0, -2, 4));
    CHECK(is(scan({0.9f}, 0.5, {-3}, 5, 0, 10, 0), 1, 1, 0, 0, 3, 9));
    // neighbours at distance 2 m + 1: 110 belongs to label 0's window [100, 110], 120 to label 1's [111, 121]
    CHECK(is(scan(v, 0.5, {105, 116}, 5, 100, 10, 0), 5, 2, 3, 0, 5 + 4, 25 + 16));
    // the hit bit belongs to the label: a second label hit after a repeat of the first
    CHECK(is(scan({0.9f, 0.9f, 0.9f, 0.9f}, 0.5, {105, 130}, 6, 100, 10, 0), 4, 2, 1, 1, -5 + 0, 25));
    // NaN never fires; +inf and -inf
    const std::vector<float> w = {nan, inf, -inf, 0.5f};
    CHECK(is(scan(w, 0.5, {}, 0, 0, 1, 0), 2, 0, 2, 0, 0, 0));
    CHECK(is(scan(w, -(double)inf, {}, 0, 0, 1, 0), 3, 0, 3, 0, 0, 0));          // everything but NaN
    CHECK(is(scan(w, (double)inf, {}, 0, 0, 1, 0), 1, 0, 1, 0, 0, 0));           // +inf only
    CHECK(is(scan(w, 1e39, {}, 0, 0, 1, 0), 1, 0, 1, 0, 0, 0));                  // beyond FLT_MAX: +inf only
    CHECK(is(scan(w, -1e39, {}, 0, 0, 1, 0), 2, 0, 2, 0, 0, 0));                 // -inf is below it
    // the float threshold is the smallest float >= theta
    const double x = (double)0.3f;
    CHECK(sd::score_threshold_f32(x) == 0.3f);
    CHECK(sd::score_threshold_f32(std::nextafter(x, 1.0)) == std::nextafterf(0.3f, 1.0f));
    CHECK(sd::score_threshold_f32(std::nextafter(x, 0.0)) == 0.3f);
    CHECK(sd::score_threshold_f32(1e39) == inf && sd::score_threshold_f32(-1e39) == -std::numeric_limits<float>::max());
    CHECK(sd::score_threshold_f32(-(double)inf) == -inf && sd::score_threshold_f32((double)inf) == inf);
    CHECK(sd::score_threshold_f32(1e-60) == std::numeric_limits<float>::denorm_min() && sd::score_threshold_f32(-1e-60) == 0.0f);
    std::printf(failures ? "FAILED\n" : "ok\n");
    return failures ? 1 : 0;
}
