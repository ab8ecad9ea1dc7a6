// match_classes_test.cpp -- csrc/match_classes.hpp alone (no library, no device), built by tests/test_match_bank_host.py under ASan
// and UBSan: the class score is the greatest of the class's template scores and `which` the lowest template that attains it,
// against the header's words written as two loops; NaN positions give NaN and -1; arrays on the heap exactly as long as the header
// says, so a read or a write outside them is caught.  Prints "ok".
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "match_classes.hpp"

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

static uint32_t bits(float v)
{
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

int main()
{
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // one step after another
    float run;
    int32_t w;
    sd::match_class_begin(run, w);
    CHECK(run != run && w == -1);
    sd::match_class_take(nan, 0, run, w);
    CHECK(run != run && w == -1);                                  // a NaN is never taken
    sd::match_class_take(-inf, 1, run, w);
    CHECK(run == -inf && w == 1);                                  // the first value, whatever it is
    sd::match_class_take(0.5f, 2, run, w);
    sd::match_class_take(0.5f, 3, run, w);
    CHECK(run == 0.5f && w == 2);                                  // a tie keeps the lower template
    sd::match_class_take(nan, 4, run, w);
    sd::match_class_take(0.25f, 5, run, w);
    CHECK(run == 0.5f && w == 2);
    sd::match_class_take(inf, 6, run, w);
    CHECK(run == inf && w == 6);

    // whole planes against two loops: few distinct values so that ties abound, columns that are all NaN, all +0.0
    const float pool[] = {0.25f, 0.5f, 0.5f, 0.75f, 0.0f, 0.0f, -1.0f, 0.9f, inf, -inf};
    for (int K : {1, 2, 5, 17, sd::kMatchMaxTemplates})
        for (int C : {1, 2, 3, sd::kMatchMaxClasses}) {
            if (C > K) continue;
            for (int64_t P : {0, 1, 7, 300}) {
                for (int table = 0; table < 2; table++) {
                    if (table == 0 && C != K) continue;            // NULL: template k is class k
                    std::vector<int32_t> cls((size_t)K);
                    for (int k = 0; k < K; k++) cls[(size_t)k] = k < C ? k : (int32_t)(draw() % (uint32_t)C);
                    for (int k = K - 1; k > 0; k--) std::swap(cls[(size_t)k], cls[(size_t)(draw() % (uint32_t)(k + 1))]);
                    std::vector<float> s((size_t)(K * P)), out((size_t)(C * P), 7.0f);
                    std::vector<int32_t> which((size_t)(C * P), 99);
                    for (int64_t p = 0; p < P; p++) {
                        const int kind = (int)(draw() % 8u);       // 0: every template NaN there; 1: every template +0.0
                        for (int k = 0; k < K; k++) s[(size_t)(k * P + p)] = kind == 0 ? nan : kind == 1 ? 0.0f : pool[draw() % 10u];
                    }
                    sd::match_classes(s.data(), P, K, table ? cls.data() : nullptr, C, out.data(), which.data());
                    std::vector<float> alone((size_t)(C * P), 7.0f);
                    sd::match_classes(s.data(), P, K, table ? cls.data() : nullptr, C, alone.data(), nullptr);
                    CHECK(P == 0 || std::memcmp(alone.data(), out.data(), (size_t)(C * P) * 4) == 0);
                    for (int c = 0; c < C; c++)
                        for (int64_t p = 0; p < P; p++) {
                            int best = -1;
                            for (int k = 0; k < K; k++) {          // the greatest; of equals the lowest k
                                if ((table ? cls[(size_t)k] : k) != c) continue;
                                const float v = s[(size_t)(k * P + p)];
                                if (v != v) continue;
                                if (best < 0 || v > s[(size_t)(best * P + p)]) best = k;
                            }
                            const float got = out[(size_t)(c * P + p)];
                            CHECK(which[(size_t)(c * P + p)] == best);
                            if (best < 0) CHECK(got != got);
                            else CHECK(bits(got) == bits(s[(size_t)(best * P + p)]));
                        }
                }
            }
        }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
