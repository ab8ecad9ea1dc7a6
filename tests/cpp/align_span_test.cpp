// align_span_test.cpp -- csrc/align_span.hpp on the host, alone (no HIP, no library): built with -fsanitize=address,undefined by
// tests/test_align_host.py and run as a program of its own.  It walks align_span over every event of the grid the GPU tests use
// -- the two clocks (hop 132 and 131: need 256, T 10), the recording lengths, the fixed and the seeded random events, the (before,
// after) pairs, the three sources -- and checks
//   1. the floor division against a definition by search, for negative numerators too
//   2. that no unit of a span leaves [0, U): 0 <= unit, unit + count <= U, first + count <= n
//   3. the span against a walk over the window unit by unit (which units lie in [0, U))
//   4. a copy through the span, as the host function and the kernel make it, out of a heap block of exactly U x width floats: a
//      read outside it is an AddressSanitizer report, an overflow in the arithmetic a UBSan report
// Prints "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "align_span.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0)
{
    if (ok) return;
    if (failures++ < 20) std::fprintf(stderr, "FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
}

struct Clock {
    int64_t hop, need, T;
    int64_t first_index() const { return (T - 1) * hop + need; }
    int64_t frames(int64_t n) const { return n < need ? 0 : (n - need) / hop + 1; }
    int64_t evals(int64_t n) const { return frames(n) >= T ? frames(n) - T + 1 : 0; }
};

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

}  // namespace

int main()
{
    // 1. the floor division
    for (int64_t b : {1, 2, 3, 131, 132, 1000}) {
        for (int64_t a = -3000; a <= 3000; a++) {
            int64_t q = -4000;
            while ((q + 1) * b <= a) q++;                                // the greatest q with q b <= a
            expect(sd::align_floor_div(a, b) == q, "floor division", a, b, sd::align_floor_div(a, b));
        }
    }
    const int64_t lim = sd::kAlignEventLimit - 1;
    expect(sd::align_floor_div(-lim, 132) * 132 <= -lim && (sd::align_floor_div(-lim, 132) + 1) * 132 > -lim, "floor division at -(2^62 - 1)");
    expect(sd::align_floor_div(lim, 131) * 131 <= lim && (sd::align_floor_div(lim, 131) + 1) * 131 > lim, "floor division at 2^62 - 1");

    const Clock clocks[] = {{132, 256, 10}, {131, 256, 10}};
    const int64_t lengths[] = {0, 255, 256, 387, 388, 1443, 1444, 1575, 1576, 5000, 12001, 30011};
    long long spans = 0, states[5] = {0, 0, 0, 0, 0};
    for (const Clock &c : clocks) {
        const int64_t pairs[][2] = {{0, 0}, {c.T - 1, 0}, {0, 5}, {7, 9}, {300, 300}, {0, 3}, {1, 2}, {2, 1}, {3, 0}};
        for (int source = 0; source < 3; source++) {
            const int64_t origin = source == sd::kAlignColumns ? c.need : source == sd::kAlignOutputs ? c.first_index() : 0;
            const int64_t step = source == sd::kAlignSamples ? 1 : c.hop;
            const int width = source == sd::kAlignColumns ? 30 : 1;     // (a band of 30 bins; the sample network's has 29: the span does not care)
            for (int64_t n : lengths) {
                const int64_t U = source == sd::kAlignColumns ? c.frames(n) : source == sd::kAlignOutputs ? c.evals(n) : n;
                std::vector<int64_t> events = {-5000, -1, 0, c.need - 1, c.need, c.first_index() - 1, c.first_index(), c.first_index() + c.hop - 1,
                                               c.first_index() + c.hop, c.first_index() + (c.evals(n) > 0 ? c.evals(n) - 1 : 0) * c.hop, n - 1, n,
                                               n + 1000000, lim, -lim};
                for (int i = 0; i < 20; i++) events.push_back((int64_t)(rng() % (uint64_t)(n + 2001)) - 1000);
                // the detector's units in a heap block of their own: unit u holds u * width + k
                float *block = (float *)std::malloc((size_t)(U * width > 0 ? U * width : 1) * sizeof(float));
                for (int64_t i = 0; i < U * width; i++) block[i] = (float)i;
                for (const auto &pr : pairs) {
                    const int64_t before = pr[0], after = pr[1], units = before + after + 1;
                    std::vector<float> window((size_t)(units * width));
                    for (int64_t s : events) {
                        const sd::AlignSpan sp = sd::align_span(s, origin, step, before, after, U);
                        spans++;
                        expect(sp.count >= 0 && sp.first >= 0 && sp.unit >= 0 && sp.first + sp.count <= units, "a span outside its window", s, sp.first, sp.count);
                        expect(sp.unit + sp.count <= U, "a span outside [0, U)", s, sp.unit + sp.count, U);
                        // unit by unit
                        const int64_t u0 = sd::align_floor_div(s - origin, step);
                        int64_t first = -1, count = 0;
                        for (int64_t j = 0; j < units; j++) {
                            const int64_t u = u0 - before + j;
                            if (u < 0 || u >= U) continue;
                            if (first < 0) first = j;
                            count++;
                        }
                        expect(count == sp.count && (count == 0 || (first == sp.first && u0 - before + first == sp.unit)), "a span that is not the window's present units", s, count, sp.count);
                        states[count == units ? 0 : count == 0 ? 4 : (sp.first > 0 ? 1 : 0) + (sp.first + sp.count < units ? 2 : 0)]++;
                        // the copy
                        for (float &v : window) v = -7.0f;
                        if (sp.count > 0) std::memcpy(window.data() + sp.first * width, block + sp.unit * width, (size_t)(sp.count * width) * sizeof(float));
                        for (int64_t j = 0; j < units; j++) {
                            const int64_t u = u0 - before + j;
                            for (int k = 0; k < width; k++) {
                                const float want = u >= 0 && u < U ? (float)(u * width + k) : -7.0f;
                                if (window[(size_t)(j * width + k)] != want) {
                                    expect(false, "a window element", s, j, k);
                                    j = units;
                                    break;
                                }
                            }
                        }
                    }
                }
                std::free(block);
            }
        }
    }
    // wholly present, clipped on the left, on the right, on both sides, wholly absent: the grid holds every state
    for (int i = 0; i < 5; i++) expect(states[i] > 0, "a state the grid never reaches", i);
    if (failures) {
        std::fprintf(stderr, "%d failures in %lld spans\n", failures, spans);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
