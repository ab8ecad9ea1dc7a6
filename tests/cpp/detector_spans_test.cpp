// The one detector table (csrc/detector_spans.hpp) on its own: the unit rules, the bounds rule, the by_row table and the lookup
// the kernels run -- the header's own text, its qualifiers taken away for the host -- against brute force over seeded random plans.
// Built with -fsanitize=address,undefined by tests/test_detector_spans_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "detector_spans.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) std::printf("line %d (plan %d): %s\n", __LINE__, trial, #c); failures++; } } while (0)
static int trial = -1;
// what the plans held, counted over all of them
static long n_in_samples = 0, n_ties = 0, n_lookups = 0, n_found = 0, n_kind[5] = {0, 0, 0, 0, 0};

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd()                                            // xorshift64*
{
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return state * 0x2545f4914f6cdd1dull;
}
static int64_t below(int64_t n) { return (int64_t)(rnd() % (uint64_t)n); }

// the sample network's clock: windows of 256 samples every 132, 10 columns an evaluation
static sd::BankInfo clock_of(int rows)
{
    sd::BankInfo b{};
    b.channels = rows;
    b.window_length = 256;
    b.time_range = 10;
    b.geom.hop = 132;
    b.geom.gap = 0;
    return b;
}

// the detector that holds unit q of `row` (tail 0: e - first < units) or a window of n units from q on (tail 1: q + n <= first +
// units), by the lookup and the caller's tail condition as train_targets_kernel and match_position state them; -1: none
static int by_lookup(const std::vector<sd::DetSpan> &by_row, const std::vector<int32_t> &row_begin, int row, int64_t q, int tail, int64_t n)
{
    const int at = sd::span_at_or_before(by_row.data(), row_begin.data(), row, q);
    if (at < 0) return -1;
    const sd::DetSpan e = by_row[(size_t)at];
    const bool has = tail == 0 ? q - e.first < e.units : q + n <= e.first + e.units;
    return has ? e.det : -1;
}
// ... and by a scan over the spans in the caller's order (spans that have units are disjoint: at most one holds q)
static int by_scan(const std::vector<sd::DetSpan> &spans, int row, int64_t q, int tail, int64_t n)
{
    int found = -1, count = 0;
    for (const sd::DetSpan &e : spans) {
        if (e.row != row || q < e.first || q >= e.first + e.units) continue;
        count++;
        if (tail == 0 || q + n <= e.first + e.units) found = e.det;
    }
    if (count > 1) {                                             // (the plans below never overlap two spans)
        std::printf("plan %d: two spans hold unit %lld of row %d\n", trial, (long long)q, row);
        failures++;
    }
    return found;
}

static void one_plan()
{
    const int rows = 1 + (int)below(8), K = (int)below(41);
    const sd::BankInfo b = clock_of(rows);
    // lengths: no samples, less than a frame, frames but no evaluation, a few evaluations, long ones
    std::vector<syldet_slot_t> plan((size_t)K);
    std::vector<int64_t> fill((size_t)rows, 0);
    bool any_squeezed = false;
    for (int k = 0; k < K; k++) {
        const int kind = (int)below(6);
        const int64_t ns = kind == 0 ? 0 : kind == 1 ? 1 + below(255) : kind == 2 ? 256 + below(9 * 132) : kind == 3 ? 256 + 9 * 132 + below(5 * 132) : 256 + below(6000);
        n_kind[kind < 4 ? kind : 4]++;
        syldet_slot_t &s = plan[(size_t)k];
        s.row = (int32_t)below(rows);
        // a recording of no samples takes no room, so its successor shares its first unit; now and then one of less than a frame
        // does not either (its frames and evaluations are none: nothing of it is read), which makes zero-unit spans share a first
        // unit with a non-empty one in every unit but samples
        s.offset = fill[(size_t)s.row];
        s.first_eval = s.offset / b.geom.hop;
        s.n_samples = ns;
        s.n_evals = sd::count_evals(b.geom, b.window_length, b.time_range, ns);
        const bool squeezed = kind == 1 && below(4) == 0;
        any_squeezed = any_squeezed || squeezed;
        if (!squeezed) fill[(size_t)s.row] += (ns + b.geom.hop - 1) / b.geom.hop * b.geom.hop;
    }
    int64_t row_samples = 0;
    for (int64_t f : fill) row_samples = f > row_samples ? f : row_samples;
    row_samples = (row_samples + 7) / 8 * 8;
    const int64_t row_evals = sd::count_evals(b.geom, b.window_length, b.time_range, row_samples);

    for (int u = 0; u < 3; u++) {
        const sd::SpanUnit unit = u == 0 ? sd::kSpanSamples : u == 1 ? sd::kSpanFrames : sd::kSpanEvals;
        if (unit == sd::kSpanSamples && any_squeezed) continue;      // (in samples such a recording overlaps its successor)
        const int64_t row_units = sd::span_row_units(b, unit, row_samples, row_evals);
        std::vector<sd::DetSpan> spans;
        for (int k = 0; k < K; k++) spans.push_back(sd::span_of(plan[(size_t)k], k, b, unit));
        n_in_samples += u == 0;
        for (const sd::DetSpan &x : spans)
            for (const sd::DetSpan &y : spans) n_ties += x.row == y.row && x.first == y.first && x.units == 0 && y.units > 0;
        // the unit rules
        CHECK(row_units == (u == 0 ? row_samples : u == 1 ? sd::count_frames(b.geom, b.window_length, row_samples) : row_evals));
        for (int k = 0; k < K; k++) {
            const syldet_slot_t &p = plan[(size_t)k];
            const sd::DetSpan &e = spans[(size_t)k];
            CHECK(e.det == k && e.row == p.row);
            if (u == 0) CHECK(e.first == p.offset && e.units == p.n_samples);
            if (u == 1) CHECK(e.first == p.first_eval && e.units == sd::count_frames(b.geom, b.window_length, p.n_samples) && e.units >= 0);
            if (u == 2) CHECK(e.first == p.first_eval && e.units == p.n_evals);
            if (u == 1 && p.n_samples < 256) CHECK(e.units == 0);
            if (u == 2 && p.n_samples < 256 + 9 * 132) CHECK(e.units == 0);
            if (u == 2 && p.n_samples >= 256 + 9 * 132) CHECK(e.units == (p.n_samples - 256) / 132 + 1 - 9);
        }
        // the bounds rule takes the plan, zero-unit spans anywhere included ...
        CHECK(sd::spans_first_beyond(spans.data(), K, rows, row_units) == -1);
        if (K > 0) {
            std::vector<sd::DetSpan> bad = spans;
            const size_t z = (size_t)below(K);
            bad[z].units = 0;
            bad[z].first = below(2) ? -5 : row_units + 7;
            CHECK(sd::spans_first_beyond(bad.data(), K, rows, row_units) == -1);
            // ... and names the first offender: a bad row, a negative first, an overrun (behind a second, later offender)
            for (int what = 0; what < 4; what++) {
                bad = spans;
                const int64_t at = below(K), later = at + below(K - at);
                for (int64_t k : {later, at}) {
                    sd::DetSpan &e = bad[(size_t)k];
                    if (what == 0) e.row = rows;
                    if (what == 1) e.row = -1;
                    if (what >= 2 && e.units == 0) e.units = 1;
                    if (what == 2) e.first = -1;
                    if (what == 3) e.first = row_units - e.units + 1;
                }
                CHECK(sd::spans_first_beyond(bad.data(), K, rows, row_units) == at);
            }
        }
        // the by_row table: a permutation of the input in (row, first, units) order, row_begin the prefix of the rows' counts
        std::vector<sd::DetSpan> by_row;
        std::vector<int32_t> row_begin;
        sd::spans_by_row(spans, rows, &by_row, &row_begin);
        CHECK(by_row.size() == spans.size() && row_begin.size() == (size_t)rows + 1 && row_begin[0] == 0 && row_begin[(size_t)rows] == K);
        std::vector<int> seen((size_t)K, 0);
        for (const sd::DetSpan &e : by_row) {
            CHECK(e.det >= 0 && e.det < K);
            const sd::DetSpan &o = spans[(size_t)e.det];
            CHECK(o.first == e.first && o.units == e.units && o.row == e.row && o.det == e.det);
            seen[(size_t)e.det]++;
        }
        for (int k = 0; k < K; k++) CHECK(seen[(size_t)k] == 1);
        for (int c = 0; c < rows; c++) {
            int count = 0;
            for (const sd::DetSpan &e : spans) count += e.row == c;
            CHECK(row_begin[(size_t)c + 1] - row_begin[(size_t)c] == count);
            for (int i = row_begin[(size_t)c]; i < row_begin[(size_t)c + 1]; i++) {
                CHECK(by_row[(size_t)i].row == c);
                if (i > row_begin[(size_t)c]) {
                    const sd::DetSpan &x = by_row[(size_t)i - 1], &y = by_row[(size_t)i];
                    CHECK(x.first < y.first || (x.first == y.first && x.units <= y.units));
                    if (x.first == y.first && x.units == y.units) CHECK(x.det < y.det);          // (stable)
                }
            }
        }
        // the lookup and each caller's tail condition against the scan, at every unit of every row and one on either side
        // (whole rows in frames and evaluations; in samples the rows' ends and every span's ends, which is where it can go wrong)
        for (int c = 0; c < rows; c++) {
            std::vector<int64_t> qs;
            if (u == 0) {
                for (const sd::DetSpan &e : spans)
                    for (int64_t dq = -2; dq <= 2; dq++) {
                        qs.push_back(e.first + dq);
                        qs.push_back(e.first + e.units + dq);
                    }
                for (int64_t dq = -1; dq <= 1; dq++) qs.push_back(dq), qs.push_back(row_units - 1 + dq);
            } else {
                for (int64_t q = -1; q <= row_units; q++) qs.push_back(q);
            }
            for (int64_t q : qs) {
                n_lookups++;
                n_found += by_scan(spans, c, q, 0, 0) >= 0;
                CHECK(by_lookup(by_row, row_begin, c, q, 0, 0) == by_scan(spans, c, q, 0, 0));
                for (int64_t n : {(int64_t)1, (int64_t)12, 1 + below(40)})
                    CHECK(by_lookup(by_row, row_begin, c, q, 1, n) == by_scan(spans, c, q, 1, n));
            }
        }
    }
}

int main()
{
    for (trial = 0; trial < 300; trial++) one_plan();
    trial = -1;
    std::printf("%ld plans in samples, %ld zero-unit spans at a non-empty one's first unit, %ld units looked up (%ld inside a span), lengths %ld %ld %ld %ld %ld\n",
                n_in_samples, n_ties, n_lookups, n_found, n_kind[0], n_kind[1], n_kind[2], n_kind[3], n_kind[4]);
    CHECK(n_in_samples >= 50 && n_ties >= 500 && n_lookups >= 100000 && n_found >= n_lookups / 10 && n_found <= n_lookups * 9 / 10);
    for (int k = 0; k < 5; k++) CHECK(n_kind[k] >= 500);
    // zero-unit spans that share a first unit with a non-empty one, by hand: the lookup lands on the one that has units
    {
        const std::vector<sd::DetSpan> spans = {{7, 0, 0, 0}, {7, 5, 1, 0}, {7, 0, 2, 0}, {12, 0, 3, 0}, {0, 7, 4, 0}, {12, 3, 5, 0}};
        std::vector<sd::DetSpan> by_row;
        std::vector<int32_t> row_begin;
        sd::spans_by_row(spans, 1, &by_row, &row_begin);
        const int order[6] = {4, 0, 2, 1, 3, 5};
        for (int i = 0; i < 6; i++) CHECK(by_row[(size_t)i].det == order[i]);
        const int holds[17] = {-1, 4, 4, 4, 4, 4, 4, 4, 1, 1, 1, 1, 1, 5, 5, 5, -1};     // q = -1 .. 15
        for (int q = -1; q <= 15; q++) CHECK(by_lookup(by_row, row_begin, 0, q, 0, 0) == holds[q + 1]);
        CHECK(by_lookup(by_row, row_begin, 0, 7, 1, 5) == 1 && by_lookup(by_row, row_begin, 0, 8, 1, 5) == -1);
        CHECK(sd::spans_first_beyond(spans.data(), 6, 1, 15) == -1 && sd::spans_first_beyond(spans.data(), 6, 1, 14) == 5);
    }
    // a table without rows or spans
    {
        std::vector<sd::DetSpan> by_row;
        std::vector<int32_t> row_begin;
        sd::spans_by_row({}, 3, &by_row, &row_begin);
        CHECK(by_row.empty() && row_begin == std::vector<int32_t>(4, 0));
        for (int c = 0; c < 3; c++) CHECK(sd::span_at_or_before(by_row.data(), row_begin.data(), c, 5) == -1);
        CHECK(sd::spans_first_beyond(nullptr, 0, 3, 0) == -1);
    }
    if (failures == 0) std::printf("ok\n");
    else std::printf("%d failures\n", failures);
    return failures != 0;
}
