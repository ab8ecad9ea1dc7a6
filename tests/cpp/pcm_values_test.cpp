// pcm_values_test.cpp -- csrc/pcm_values.hpp on the host, alone (no HIP, no library): built with -fsanitize=address,undefined by
// tests/test_recordings_pcm_host.py and run as a program of its own.  Every buffer is a heap block that ends with the last sample
// byte, so a read past a recording's samples -- by pcm_value or by the group-of-four path -- is an AddressSanitizer report.
//   1. hand-worked values of every format
//   2. every format, at byte offsets 0 to 3 inside its block and at every step a file of 1, 2 or 3 tracks gives (S24: 3, 6, 9):
//      pcm_value against an independent decode written here byte by byte
//   3. the group-of-four path over the same blocks: wherever four contiguous samples remain, at every address the offsets give --
//      equal to pcm_value sample by sample, the blocks' ends included
// Prints "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "pcm_values.hpp"

namespace {

int failures = 0;

uint32_t bits(float f)
{
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

void expect(bool ok, const char *what, long a = 0, long b = 0, long c = 0)
{
    if (ok) return;
    if (failures++ < 20) std::fprintf(stderr, "FAILED: %s (%ld, %ld, %ld)\n", what, a, b, c);
}

// NaNs in the same places, every other value by bits
bool same(float a, float b) { return (a != a && b != b) || bits(a) == bits(b); }

// the table of include/syldet.h, byte by byte and through fp64, sharing nothing with the header
float model(int format, const unsigned char *p)
{
    switch (format) {
    case sd::kPcmU8: return (float)(((double)p[0] - 128.0) / 128.0);
    case sd::kPcmS16: {
        const int v = p[0] | p[1] << 8;
        return (float)((double)(v >= 32768 ? v - 65536 : v) / 32768.0);
    }
    case sd::kPcmS24: {
        const long v = (long)p[0] | (long)p[1] << 8 | (long)p[2] << 16;
        return (float)((double)(v >= 8388608 ? v - 16777216 : v) / 8388608.0);
    }
    case sd::kPcmS32: {
        const int64_t v = (int64_t)p[0] | (int64_t)p[1] << 8 | (int64_t)p[2] << 16 | (int64_t)p[3] << 24;
        return (float)((double)(v >= 2147483648ll ? v - 4294967296ll : v) / 2147483648.0);
    }
    case sd::kPcmF32: {
        const uint32_t b = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
        float f;
        std::memcpy(&f, &b, 4);
        return f;
    }
    default: {
        uint64_t b = 0;
        for (int i = 0; i < 8; i++) b |= (uint64_t)p[i] << (8 * i);
        double d;
        std::memcpy(&d, &b, 8);
        return (float)d;
    }
    }
}

// a heap block of exactly `n` bytes (the allocator's own alignment: at least 16)
struct Block {
    unsigned char *p;
    explicit Block(size_t n) : p((unsigned char *)std::malloc(n ? n : 1)) {}
    ~Block() { std::free(p); }
};

float one(int format, std::initializer_list<unsigned> b)
{
    Block blk(b.size());
    size_t i = 0;
    for (unsigned v : b) blk.p[i++] = (unsigned char)v;
    return sd::pcm_value(format, blk.p);
}

float one_f64(double d)
{
    Block blk(8);
    std::memcpy(blk.p, &d, 8);
    return sd::pcm_value(sd::kPcmF64, blk.p);
}

void hand_worked()
{
    expect(one(sd::kPcmS24, {0x00, 0x00, 0x80}) == -1.0f, "S24 0x800000 is -1");
    expect(one(sd::kPcmS24, {0xff, 0xff, 0x7f}) == 1.0f - std::ldexp(1.0f, -23), "S24 0x7FFFFF is 1 - 2^-23");
    expect(one(sd::kPcmS24, {0xff, 0xff, 0xff}) == -std::ldexp(1.0f, -23), "S24 0xFFFFFF is -2^-23");
    // INT32_MIN + 1 = -(2^31 - 1) rounds to -2^31 in fp32: -1
    expect(one(sd::kPcmS32, {0x01, 0x00, 0x00, 0x80}) == -1.0f, "S32 INT32_MIN + 1 is -1");
    expect(one(sd::kPcmS32, {0x00, 0x00, 0x00, 0x80}) == -1.0f, "S32 INT32_MIN is -1");
    expect(one(sd::kPcmS32, {0x80, 0xff, 0xff, 0x7f}) == 1.0f - std::ldexp(1.0f, -24), "S32 2^31 - 128 is 1 - 2^-24");
    expect(one(sd::kPcmS32, {0x01, 0x00, 0x00, 0x00}) == std::ldexp(1.0f, -31), "S32 1 is 2^-31");
    expect(one(sd::kPcmS16, {0x00, 0x80}) == -1.0f && one(sd::kPcmS16, {0xff, 0x7f}) == 32767.0f / 32768.0f, "S16 ends");
    expect(one(sd::kPcmU8, {0}) == -1.0f && one(sd::kPcmU8, {128}) == 0.0f && bits(one(sd::kPcmU8, {128})) == 0u && one(sd::kPcmU8, {255}) == 127.0f / 128.0f,
           "U8 0, 128, 255");
    // 1e-40 is below FLT_MIN (1.18e-38): the fp32 subnormal nearest to it, 71362 * 2^-149
    const float sub = one_f64(1e-40);
    expect(sub > 0.0f && sub < std::numeric_limits<float>::min() && bits(sub) == 71362u, "F64 1e-40 is the fp32 subnormal 71362 * 2^-149", (long)bits(sub));
    expect(one_f64(HUGE_VAL) == HUGE_VALF && one_f64(-HUGE_VAL) == -HUGE_VALF, "F64 +-inf");
    expect(bits(one_f64(-0.0)) == 0x80000000u && bits(one_f64(0.0)) == 0u, "F64 +-0");
    expect(one_f64(1.0 + std::ldexp(1.0, -24)) == 1.0f && one_f64(1.0 + 3.0 * std::ldexp(1.0, -24)) == 1.0f + std::ldexp(1.0f, -22), "F64 ties to even");
    expect(bits(one(sd::kPcmF32, {0x45, 0x23, 0xc1, 0x7f})) == 0x7fc12345u, "F32 keeps a NaN's payload");
    expect(bits(one(sd::kPcmF32, {0x01, 0x00, 0x00, 0x00})) == 1u, "F32 keeps a subnormal");
    expect(sd::pcm_sample_bytes(0) == 0 && sd::pcm_sample_bytes(7) == 0 && sd::pcm_sample_bytes(sd::kPcmS24) == 3 && sd::pcm_sample_bytes(sd::kPcmF64) == 8,
           "sample bytes");
}

uint32_t rng_state = 12345u;
unsigned char next_byte()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (unsigned char)(rng_state >> 24);
}

void blocks()
{
    const int formats[6] = {sd::kPcmU8, sd::kPcmS16, sd::kPcmS24, sd::kPcmS32, sd::kPcmF32, sd::kPcmF64};
    for (int format : formats) {
        const int size = sd::pcm_sample_bytes(format);
        for (int tracks = 1; tracks <= 3; tracks++)
            for (int off = 0; off < 4; off++)
                for (int n : {1, 2, 3, 4, 5, 7, 8, 9, 64, 67}) {
                    const int step = tracks * size;
                    // the host reads byte-wise, so every offset is legal for every format here; on the device the typed formats
                    // only meet multiples of their size (the calls refuse the rest)
                    const size_t len = (size_t)off + (size_t)(n - 1) * step + size;       // ends with the last sample byte
                    Block blk(len);
                    for (size_t i = 0; i < len; i++) blk.p[i] = next_byte();
                    const unsigned char *first = blk.p + off;
                    std::vector<float> want((size_t)n);
                    for (int i = 0; i < n; i++) {
                        want[(size_t)i] = model(format, first + (size_t)i * step);
                        expect(same(sd::pcm_value(format, first + (size_t)i * step), want[(size_t)i]), "pcm_value against the model", format, step, i);
                    }
                    if (tracks != 1) continue;
                    // the group-of-four path wherever four samples remain: every start, so every address class and the block's end
                    for (int i = 0; i + 4 <= n; i++) {
                        float g[4];
                        sd::pcm_group4(format, first + (size_t)i * size, g);
                        for (int j = 0; j < 4; j++) expect(same(g[j], want[(size_t)(i + j)]), "pcm_group4 against the model", format, off, i + j);
                    }
                }
    }
}

}  // namespace

int main()
{
    hand_worked();
    blocks();
    if (failures) {
        std::fprintf(stderr, "%d check(s) failed\n", failures);
        return 1;
    }
    std::puts("ok");
    return 0;
}
