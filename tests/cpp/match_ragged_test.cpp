// match_ragged_test.cpp -- csrc/match_ragged.hpp alone (no library, no device), built by tests/test_match_ragged_host.py under ASan
// and UBSan: the plan of a ragged bank's tile against brute force over seeded sets of (n_k, a_k, bins) -- the lead, the tail, the
// staged frames, the floats counted region by region; the two read bounds of a pass (every frame a pass of the products or an
// energy sum reads is fetched from a heap array of exactly G elements, every LDS address from one of exactly the tile's floats, so
// a read outside them is caught); and the window rule at both ends of a span.  Prints "ok".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "match_ragged.hpp"

static int failures = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        if (!(c)) {                                                    \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);        \
            failures++;                                                \
        }                                                              \
    } while (0)

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint32_t draw()
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33);
}

static void one_bank(const std::vector<int32_t> &n, const std::vector<int32_t> &a, int bins)
{
    const int K = (int)n.size(), tile = sd::kMatchTileElements;
    const sd::MatchRaggedPlan p = sd::match_ragged_plan(n.data(), a.data(), K, bins);
    // brute force: the frames, relative to the tile's first element, that any window of any element of the tile holds
    int lo = 0, hi = 0, n_max = 0;
    for (int k = 0; k < K; k++)
        for (int e = 0; e < tile; e++)
            for (int j = 0; j < n[(size_t)k]; j++) {
                lo = std::min(lo, e - a[(size_t)k] + j);
                hi = std::max(hi, e - a[(size_t)k] + j);
            }
    for (int k = 0; k < K; k++) n_max = std::max(n_max, n[(size_t)k]);
    CHECK(p.a_max == -lo && p.G == hi - lo + 1 && p.G == tile - 1 + p.a_max + p.r_max && p.n_max == n_max);
    CHECK(p.Fp % 4 == 0 && p.Fp >= bins && p.Fp < bins + 4 && p.FT % 4 == 0 && ((p.FT / 4) & 1) == 1 && (p.FT == p.Fp || p.FT == p.Fp + 4));
    // the floats, region by region: frame g at g Fp + 4 (g >> 4); the template region; the energies; four waves' sums
    const int64_t x_floats = (int64_t)(p.G - 1) * p.Fp + 4 * ((p.G - 1) >> 4) + p.Fp;
    const int64_t x_region = (int64_t)p.G * p.Fp + 4 * ((p.G + 15) / 16);
    CHECK(x_region - x_floats == 4);                                    // (one step of the skew to spare)
    CHECK(p.floats == x_region + (int64_t)n_max * p.FT + p.G + 4 * tile);
    CHECK(p.matrix == (p.floats * 4 <= sd::kMatchLdsBytes) && p.lds_bytes == (p.matrix ? (int)(p.floats * 4) : 0));
    // one template alone with its last frame as anchor is the single matcher's tile: G = 255 + n
    for (int k = 0; k < K; k++) {
        const int32_t nk = n[(size_t)k], ak = nk - 1;
        const sd::MatchRaggedPlan s = sd::match_ragged_plan(&nk, &ak, 1, bins);
        CHECK(s.G == tile - 1 + nk && s.floats <= p.floats);            // (so a matrix-form bank's templates are matrix-form alone)
        CHECK(s.floats == sd::match_tile_floats(tile - 1 + nk, nk, bins, nullptr, nullptr));
    }
    if (!p.matrix) return;
    // the reads: heap arrays of exactly the plan's sizes
    std::vector<int> frames((size_t)p.G, 0);
    std::vector<float> X((size_t)x_region, 0.0f), T((size_t)n_max * (size_t)p.FT, 0.0f);
    for (int k = 0; k < K; k++) {
        const int nk = n[(size_t)k], s = sd::match_ragged_first(p, a[(size_t)k]);
        CHECK(s >= 0 && s == p.a_max - a[(size_t)k]);
        int last = 0;
        for (int m = 0; m < 16; m++)
            for (int f = 0; f < nk + 15; f++)
                for (int bg = 0; bg < p.Fp / 4; bg++)
                    for (int kk = 0; kk < 4; kk++) {
                        const int g = 16 * m + s + f;
                        frames[(size_t)g]++;
                        last = std::max(last, g);
                        // the kernel's address: xa = X + 16 m Fp + 4 m + k, then (f + s) Fp + 4 ((f + s) >> 4) + 4 bg
                        const int64_t at = (int64_t)16 * m * p.Fp + 4 * m + kk + (int64_t)(f + s) * p.Fp + 4 * ((f + s) >> 4) + 4 * bg;
                        CHECK(at == (int64_t)g * p.Fp + 4 * (g >> 4) + 4 * bg + kk);
                        X[(size_t)at] += 1.0f;
                        const int j = f - m;                            // column m's template frame (selected where outside)
                        T[(size_t)(((unsigned)j < (unsigned)nk ? j : 0) * p.FT + kk + 4 * bg)] += 1.0f;
                    }
        for (int e = 0; e < tile; e++)
            for (int j = 0; j < nk; j++) {
                frames[(size_t)(e + s + j)]++;
                last = std::max(last, e + s + j);
            }
        CHECK(last == sd::match_ragged_last(p, nk, a[(size_t)k]) && last <= p.G - 1);
        // element e's window begins at the staged frame e + s: the frame e - a_k relative to the tile's first element
        CHECK(s - p.a_max == -a[(size_t)k]);
    }
    // the 64 lanes of an A read (m, k) hit 64 banks for any first frame s
    for (int s = 0; s <= p.a_max; s++) {
        bool bank[64] = {false};
        for (int lane = 0; lane < 64; lane++) {
            const int m = lane & 15, kk = lane >> 4, g = 16 * m + s + 3;
            bank[((int64_t)g * p.Fp + 4 * (g >> 4) + kk) & 63] = true;
        }
        CHECK(std::count(bank, bank + 64, true) == 64);
    }
    // the furthest read of the whole bank is the last staged frame, and the nearest the first
    int far = 0, near = p.G;
    for (int k = 0; k < K; k++) {
        far = std::max(far, sd::match_ragged_last(p, n[(size_t)k], a[(size_t)k]));
        near = std::min(near, sd::match_ragged_first(p, a[(size_t)k]));
    }
    CHECK(far == p.G - 1 && far == tile - 2 + p.a_max + p.r_max && near == 0);
}

int main()
{
    one_bank({1, 12, 17, 5, 12}, {0, 11, 16, 4, 11}, 7);
    one_bank({1, 12, 17, 5, 12}, {0, 3, 16, 4, 0}, 29);
    one_bank({12, 100}, {11, 99}, 29);                                  // plain: 100 frames of 29 bins do not fit
    {
        const int32_t n[2] = {12, 100}, a[2] = {11, 99};
        CHECK(!sd::match_ragged_plan(n, a, 2, 29).matrix && sd::match_ragged_plan(n, a, 1, 29).matrix);
        const int32_t n91 = 91, a90 = 90, a0 = 0;
        CHECK(sd::match_ragged_plan(&n91, &a90, 1, 29).matrix && sd::match_ragged_plan(&n91, &a0, 1, 29).matrix);
    }
    for (int round = 0; round < 200; round++) {
        const int K = 1 + (int)(draw() % 8u), bins = 1 + (int)(draw() % 40u);
        std::vector<int32_t> n((size_t)K), a((size_t)K);
        for (int k = 0; k < K; k++) {
            n[(size_t)k] = 1 + (int32_t)(draw() % (round % 4 == 0 ? 120u : 24u));
            const uint32_t kind = draw() % 4u;
            a[(size_t)k] = kind == 0 ? 0 : kind == 1 ? n[(size_t)k] - 1 : (int32_t)(draw() % (uint32_t)n[(size_t)k]);
        }
        one_bank(n, a, bins);
    }
    // the window rule: a span [first, end), every (n, a), every u around both ends
    for (int64_t first : {(int64_t)0, (int64_t)37})
        for (int64_t units : {(int64_t)0, (int64_t)1, (int64_t)5, (int64_t)12, (int64_t)40})
            for (int n = 1; n <= 14; n++)
                for (int a = 0; a < n; a++)
                    for (int64_t u = first - 3; u < first + units + 3; u++) {
                        bool in = true;                                 // every frame of the window is a frame of the span
                        for (int j = 0; j < n; j++) in = in && u - a + j >= first && u - a + j < first + units;
                        CHECK(sd::match_ragged_window(first, first + units, u, a, n) == in);
                        if (in) CHECK(u >= first && u < first + units);  // ... and then so is the anchor
                    }
    CHECK(sd::match_ragged_window(10, 22, 10, 0, 12) && !sd::match_ragged_window(10, 22, 11, 0, 12));    // exactly as long as the template
    CHECK(sd::match_ragged_window(10, 22, 21, 11, 12) && !sd::match_ragged_window(10, 22, 20, 11, 12));
    CHECK(!sd::match_ragged_window(10, 21, 21, 11, 12));                // one frame short: the front would reach the neighbour
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
