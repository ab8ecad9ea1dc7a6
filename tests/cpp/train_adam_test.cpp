// csrc/train_adam.hpp alone, as a host program (built with -ffp-contract=off under ASan and UBSan by tests/test_train_tool_host.py):
// the step against the same operations written out one by one through volatile floats, over heap arrays of exactly P elements;
// step 1 does not read the moments; a weight sum of 0 keeps the parameters' bits; the constants of a few steps.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "train_adam.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char *what)
{
    if (!ok) {
        std::printf("FAILED: %s\n", what);
        failures++;
    }
}

bool same_bits(const std::vector<float> &a, const std::vector<float> &b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0; }

uint64_t next(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return s >> 11;
}

// the stated operations, each rounded to fp32 through a volatile
void by_hand(int64_t t, double lr, double b1, double b2, double eps, double wsum, float grad, float &m, float &v, float &p)
{
    volatile float s = wsum > 0.0 ? (float)(1.0 / wsum) : 0.0f;
    volatile float g = grad * s;
    volatile float gg = g * g;
    volatile float m0 = t == 1 ? 0.0f : m, v0 = t == 1 ? 0.0f : v;
    volatile float a = (float)b1 * m0, b = (float)(1.0 - b1) * g;
    volatile float mn = a + b;
    volatile float c = (float)b2 * v0, d = (float)(1.0 - b2) * gg;
    volatile float vn = c + d;
    m = mn;
    v = vn;
    if (!(wsum > 0.0)) return;
    volatile float c1 = (float)(lr / (1.0 - std::pow(b1, (double)t))), c2 = (float)(1.0 / std::sqrt(1.0 - std::pow(b2, (double)t)));
    volatile float root = std::sqrt(vn);
    volatile float scaled = root * c2;
    volatile float den = scaled + (float)eps;
    volatile float q = mn / den;
    volatile float step = c1 * q;
    volatile float pn = p - step;
    p = pn;
}

}  // namespace

int main()
{
    using namespace sd;
    for (int P : {1, 74, 1169}) {
        uint64_t seed = 12345 + (uint64_t)P;
        std::vector<float> p((size_t)P), m((size_t)P, std::numeric_limits<float>::quiet_NaN()), v((size_t)P, std::numeric_limits<float>::infinity()), g((size_t)P);
        for (int i = 0; i < P; i++) {
            p[(size_t)i] = (float)((double)next(seed) / 9007199254740992.0 - 0.5);
            g[(size_t)i] = (float)(((double)next(seed) / 9007199254740992.0 - 0.5) * 1e-3);
        }
        std::vector<float> hp(p), hm(m), hv(v);
        for (int64_t t = 1; t <= 5; t++) {
            const double wsum = t == 3 ? 0.0 : 0.37 + 0.1 * (double)t;
            const TrainAdamStep k = train_adam_consts(t, 0.01, 0.9, 0.999, 1e-8);
            const std::vector<float> before(p);
            for (int i = 0; i < P; i++) {
                train_adam_element(k, wsum > 0.0, train_adam_scale(wsum), g[(size_t)i], &m[(size_t)i], &v[(size_t)i], &p[(size_t)i]);
                by_hand(t, 0.01, 0.9, 0.999, 1e-8, wsum, g[(size_t)i], hm[(size_t)i], hv[(size_t)i], hp[(size_t)i]);
            }
            expect(same_bits(p, hp) && same_bits(m, hm) && same_bits(v, hv), "the step is the stated operations, one rounding each");
            if (t == 1) {
                bool finite = true;
                for (int i = 0; i < P; i++) finite = finite && std::isfinite(m[(size_t)i]) && std::isfinite(v[(size_t)i]) && std::isfinite(p[(size_t)i]);
                expect(finite, "step 1 does not read the moments");
            }
            if (t == 3) expect(same_bits(p, before), "a weight sum of 0 keeps the parameters' bits");
            else expect(!same_bits(p, before), "a step moves the parameters");
            for (int i = 0; i < P; i++) g[(size_t)i] = g[(size_t)i] * 0.5f + (float)(((double)next(seed) / 9007199254740992.0 - 0.5) * 1e-3);
        }
    }
    const TrainAdamStep k1 = train_adam_consts(1, 0.01, 0.9, 0.999, 1e-8);
    expect(k1.first == 1 && k1.c1 == (float)(0.01 / (1.0 - 0.9)) && k1.c2 == (float)(1.0 / std::sqrt(1.0 - 0.999)), "the constants of step 1");
    expect(train_adam_consts(2, 0.01, 0.9, 0.999, 1e-8).first == 0, "step 2 reads the moments");
    expect(train_adam_scale(0.0) == 0.0f && train_adam_scale(-1.0) == 0.0f && train_adam_scale(std::nan("")) == 0.0f && train_adam_scale(4.0) == 0.25f, "the scale");
    expect(train_adam_mean(3.0, 0.0) == 0.0 && train_adam_mean(3.0, 4.0) == 0.75, "the mean loss");
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
