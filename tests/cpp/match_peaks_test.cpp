// match_peaks_test.cpp -- csrc/match_peaks.hpp alone (no library, no device), built by tests/test_match_host.py under ASan and UBSan:
// the key's order is the floats', the window maxima from the table of 2^k maxima are the brute-force maxima for every S and every
// position (the table exactly as long as the header says it must be, on the heap, so a read outside it is caught), and the rule
// with them is the rule written as two loops over the neighbours.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "match_peaks.hpp"

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

// the rule in the header's words: two loops over the neighbours, floats compared as floats
static bool brute(const std::vector<float> &s, int64_t p, int S, float threshold)
{
    const int64_t P = (int64_t)s.size();
    if (s[p] != s[p] || !(s[p] >= threshold)) return false;
    for (int64_t q = p - S < 0 ? 0 : p - S; q < p; q++)
        if (s[q] == s[q] && !(s[q] < s[p])) return false;
    for (int64_t q = p + 1; q <= p + S && q < P; q++)
        if (s[q] == s[q] && !(s[q] <= s[p])) return false;
    return true;
}

static std::vector<int64_t> by_table(const std::vector<float> &s, int S, float threshold)
{
    const int64_t P = (int64_t)s.size(), L = P + 2 * (int64_t)S;
    const int k = S ? sd::match_level(S) : 0;
    std::vector<uint32_t> cur((size_t)L, 0u), nxt((size_t)L, 0u), keys((size_t)P);
    for (int64_t p = 0; p < P; p++) keys[(size_t)p] = cur[(size_t)(p + S)] = sd::match_key(s[(size_t)p]);
    for (int lev = 0; lev < k; lev++) {
        const int64_t h = (int64_t)1 << lev;
        for (int64_t i = 0; i < L; i++) {
            const uint32_t a = cur[(size_t)i], b = i + h < L ? cur[(size_t)(i + h)] : 0u;
            nxt[(size_t)i] = a > b ? a : b;
        }
        cur.swap(nxt);
    }
    std::vector<int64_t> out;
    const uint32_t tk = sd::match_key(threshold);
    for (int64_t p = 0; p < P; p++)
        if (sd::match_rule(keys[(size_t)p], sd::match_left(cur.data(), p + S, S, k), sd::match_right(cur.data(), p + S, S, k), tk)) out.push_back(p);
    return out;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the key: NaN lowest, then the floats' order; the two zeros share one
    const float ordered[] = {-inf, -3.0e38f, -1.0f, -1.0e-45f, 0.0f, 1.0e-45f, 0.5f, 1.0f, 3.0e38f, inf};
    for (size_t i = 0; i + 1 < sizeof(ordered) / sizeof(ordered[0]); i++) CHECK(sd::match_key(ordered[i]) < sd::match_key(ordered[i + 1]));
    CHECK(sd::match_key(nan) == 0u && sd::match_key(-nan) == 0u && sd::match_key(-inf) > 0u);
    CHECK(sd::match_key(-0.0f) == sd::match_key(0.0f));
    for (int i = 0; i < 100000; i++) {
        uint32_t ua = draw() ^ (draw() << 16), ub = draw() ^ (draw() << 16);
        float a, b;
        __builtin_memcpy(&a, &ua, 4);
        __builtin_memcpy(&b, &ub, 4);
        if (a != a || b != b) continue;
        CHECK((a < b) == (sd::match_key(a) < sd::match_key(b)) && (a == b) == (sd::match_key(a) == sd::match_key(b)));
    }
    // the level: the largest k with 2^k <= S
    for (int S = 1; S <= sd::kMatchMaxSeparation; S++) {
        const int k = sd::match_level(S);
        CHECK((1 << k) <= S && (2 << k) > S);
    }
    // the event number
    CHECK(sd::match_event(256, 132, 0, 11) == 256 + 11 * 132 && sd::match_event(4294967295ll, 2147483647ll, (1ll << 31) - 1, 32767) > 0);
    // the rule from the table against the two loops: plateaus, NaN runs, infinities, few distinct values so that ties abound
    const float pool[] = {0.25f, 0.5f, 0.5f, 0.75f, -0.0f, 0.0f, nan, nan, inf, -inf, 0.9f, 0.1f};
    const int seps[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 100, 4095, 4096};
    for (int P : {0, 1, 2, 3, 10, 33, 200}) {
        for (int trial = 0; trial < 6; trial++) {
            std::vector<float> s((size_t)P);
            for (int p = 0; p < P; p++) s[(size_t)p] = trial == 0 ? 0.5f : trial == 1 ? nan : pool[draw() % (trial < 4 ? 12u : 4u)];
            for (int S : seps)
                for (float threshold : {-inf, 0.3f, 0.5f, inf}) {
                    const std::vector<int64_t> got = by_table(s, S, threshold);
                    std::vector<int64_t> want;
                    for (int p = 0; p < P; p++)
                        if (brute(s, p, S, threshold)) want.push_back(p);
                    CHECK(got == want);
                }
        }
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
