// The output gain's exact reciprocal (csrc/exact_reciprocal.hpp) on the host: which gains get one, and that where one is returned
// x * r has the bits of x / g -- for every power of two the function accepts and random x of every kind (random bit patterns:
// subnormals, huge values, infinities, products that overflow or go subnormal), each operation rounded to float on its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>

#include "exact_reciprocal.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { if (failures < 20) std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

int main()
{
    const float inf = std::numeric_limits<float>::infinity();
    CHECK(sd::exact_reciprocal_f32(2.0f) == 0.5f);
    CHECK(sd::exact_reciprocal_f32(0.5f) == 2.0f);
    CHECK(sd::exact_reciprocal_f32(-4.0f) == -0.25f);
    CHECK(sd::exact_reciprocal_f32(1.0f) == 1.0f);
    CHECK(sd::exact_reciprocal_f32(std::ldexp(1.0f, -126)) == std::ldexp(1.0f, 126));
    CHECK(sd::exact_reciprocal_f32(std::ldexp(1.0f, 126)) == std::ldexp(1.0f, -126));
    CHECK(sd::exact_reciprocal_f32(std::ldexp(1.0f, 127)) == 0.0f);          // (its reciprocal is subnormal)
    CHECK(sd::exact_reciprocal_f32(std::ldexp(1.0f, -127)) == 0.0f);         // (subnormal itself)
    CHECK(sd::exact_reciprocal_f32(3.0f) == 0.0f);
    CHECK(sd::exact_reciprocal_f32(std::nextafterf(2.0f, inf)) == 0.0f);
    CHECK(sd::exact_reciprocal_f32(std::nextafterf(2.0f, 0.0f)) == 0.0f);
    CHECK(sd::exact_reciprocal_f32(0.0f) == 0.0f && sd::exact_reciprocal_f32(-0.0f) == 0.0f);
    CHECK(sd::exact_reciprocal_f32(inf) == 0.0f && sd::exact_reciprocal_f32(-inf) == 0.0f);
    CHECK(sd::exact_reciprocal_f32(std::numeric_limits<float>::quiet_NaN()) == 0.0f);

    std::mt19937_64 rng(20240607u);
    for (int sign = 0; sign < 2; sign++)
        for (int e = -126; e <= 126; e++) {
            const float g = sign ? -std::ldexp(1.0f, e) : std::ldexp(1.0f, e), r = sd::exact_reciprocal_f32(g);
            CHECK(r != 0.0f);
            for (int i = 0; i < 4000; i++) {
                const uint32_t b = (uint32_t)rng();
                float x;
                std::memcpy(&x, &b, 4);
                if (std::isnan(x)) continue;
                volatile float q = x / g, p = x * r;             // (each rounded to float on its own)
                const float qf = q, pf = p;
                if (std::memcmp(&qf, &pf, 4) != 0) {
                    if (failures < 20) std::printf("x %.9g / %.9g = %.9g, but x * %.9g = %.9g\n", (double)x, (double)g, (double)qf, (double)r, (double)pf);
                    failures++;
                }
            }
        }
    // any other gain: no reciprocal (random bit patterns; a power of two turns up once in 2^23 draws and is skipped)
    for (int i = 0; i < 200000; i++) {
        const uint32_t b = (uint32_t)rng();
        float g;
        std::memcpy(&g, &b, 4);
        if ((b & 0x7fffffu) == 0) continue;
        CHECK(sd::exact_reciprocal_f32(g) == 0.0f);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
