// sinc_taps.hpp -- what every kernel of the band-limited converter shares (kernels_sinc.hip: the whole-recording and the streaming
// form; kernels_recordings_sinc.hip: the packed recordings' load): the LDS layout, the widening of a sample and the tap loop.  The
// kernels' bits are the same because their tap arithmetic is this one function, compiled with the same flags (-ffp-contract=off,
// see the Makefile).  Device code only; gfx950, wave = 64.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sd {

namespace {

template <typename T> __device__ __forceinline__ float sinc_sample(T v);
template <> __device__ __forceinline__ float sinc_sample<float>(float v) { return v; }
template <> __device__ __forceinline__ float sinc_sample<int16_t>(int16_t v) { return (float)v * (1.0f / 32768.0f); }

// The kernels' dynamic LDS: the table g [N + 4] (g[N] = 0: sinc(Z) = 0, then zeros), then the staged samples xs [kSincStage].
extern __shared__ __attribute__((aligned(16))) unsigned char sinc_smem[];

// What the LDS allows, told to the compiler: 80 KB a workgroup of four waves is two waves a SIMD, 144 KB one.  Without it the
// scheduler guards an occupancy of six that the LDS never grants and, to save registers, leaves some of the unrolled tap loops
// waiting for each table read in turn instead of keeping four in flight -- which ones changes with unrelated edits (3.5 ms a loop
// at 64 channels x 2^24 samples; MEASUREMENTS.md, "The streaming band-limited resampler").
#define SINC_WAVES_PER_SIMD __attribute__((amdgpu_waves_per_eu(1, 2)))

// The taps k = ka .. ka + n - 1 of one output, k ascending, added to its running sum a: xs[x0] is staged sample ka, m =
// floor(p) - ka, f = float(p - floor(p)).  Every kernel's arithmetic is this function: their bits are the same by construction.
// (It names the LDS itself instead of taking pointers, so that the compiler sees LDS accesses when it shapes the loop.)
__device__ __forceinline__ float sinc_taps(int N, int x0, int n, int m, float f, float idx_scale, float n_f, float a)
{
    const float *g = reinterpret_cast<const float *>(sinc_smem);
    const float *x = g + (N + 4) + x0;
#pragma unroll 4                                             // (the shape the loop had inside the kernel: four taps and a remainder)
    for (int q = 0; q < n; q++, m--) {
        const float t = (float)m + f;
        const float u = fminf(fabsf(t) * idx_scale, n_f);
        const int j = (int)u;                                // 0 .. N; g[N + 1] is a zero
        const float w = u - (float)j;
        const float g0 = g[j], g1 = g[j + 1];
        const float c = g0 + w * (g1 - g0);
        a = a + x[q] * c;
    }
    return a;
}

}  // namespace

}  // namespace sd
