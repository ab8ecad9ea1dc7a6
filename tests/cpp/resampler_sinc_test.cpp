// resampler_sinc_test.cpp -- syldetxx::ResamplerSinc (include/syldet.hpp) against the C ABI's whole-recording call: one row of
// 3000 samples at 48 kHz converted to 44.1 kHz in three pushes (host buffers) and a flush must be, bit for bit, what
// syldet_convert_rate_sinc_device makes of the row in one call.  Prints "ok" and exits 0; 2 without a device.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "syldet.hpp"

int main()
{
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) { std::printf("no-device\n"); return 2; }
    const double ri = 48000.0, ro = 44100.0;
    const int64_t n = 3000;
    std::vector<float> x((size_t)n);
    uint32_t seed = 12345u;
    for (float &v : x) { seed = seed * 1664525u + 1013904223u; v = (float)(seed >> 8) * (2.0f / 16777216.0f) - 1.0f; }

    // the C call on the whole row
    int32_t Z = 0;
    double beta = 0.0, rolloff = 0.0;
    syldet_sinc_defaults(&Z, &beta, &rolloff);
    const int64_t n_out = syldet_convert_rate_count(n, ri, ro);
    float *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc((void **)&d_in, (size_t)n * sizeof(float)) != hipSuccess || hipMalloc((void **)&d_out, (size_t)n_out * sizeof(float)) != hipSuccess) return 3;
    if (hipMemcpy(d_in, x.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return 3;
    int64_t got = 0;
    if (syldet_convert_rate_sinc_device(d_in, n, n, 1, ri, ro, Z, beta, rolloff, d_out, n_out, &got, nullptr) != SYLDET_OK || got != n_out) return 4;
    std::vector<float> want((size_t)n_out);
    if (hipMemcpy(want.data(), d_out, (size_t)n_out * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 3;
    (void)hipFree(d_in);
    (void)hipFree(d_out);

    // the mirror, three pushes and a flush
    std::vector<float> have;
    try {
        syldetxx::ResamplerSinc r(ri, ro);
        const int64_t cuts[4] = {0, 31, 1500, n};
        for (int b = 0; b < 3; b++) {
            const std::vector<float> part(x.begin() + cuts[b], x.begin() + cuts[b + 1]);
            const int64_t expect = r.countOutput((int64_t)part.size());
            const std::vector<float> y = r.resampleArray(part);
            if ((int64_t)y.size() != expect) return 5;
            have.insert(have.end(), y.begin(), y.end());
        }
        if (r.samplesIn() != n || r.samplesOut() != (int64_t)have.size() || r.finished()) return 6;
        const std::vector<float> tail = r.flush();
        have.insert(have.end(), tail.begin(), tail.end());
        if (!r.finished() || r.samplesOut() != n_out) return 6;
        r.reset();
        if (r.finished() || r.samplesIn() != 0) return 6;
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        return 7;
    }
    if (have.size() != want.size() || std::memcmp(have.data(), want.data(), want.size() * sizeof(float)) != 0) {
        std::printf("the pushes' outputs differ from the whole-recording call's\n");
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
