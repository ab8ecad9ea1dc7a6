// kernels_sinc.hip -- band-limited whole-recording rate conversion (the sinc convention of include/syldet.h), the step the
// reference's tool leaves to AVFoundation (audioSettings, Common/SyllableDetector.swift:19-23, handed to
// AVAssetReaderTrackOutput at SyllableDetectorCLI/TrackDetector.swift:35):
//   convert_rate_sinc_kernel<float>     fp32 rows in, fp32 rows out
//   convert_rate_sinc_kernel<int16_t>   16-bit PCM rows in (x means float(x) * 2^-15), the same arithmetic on the same floats
//   convert_rate_sinc_stream_kernel<T>  the same outputs block by block (ResamplerSinc): what was kept plus what just arrived
//   sinc_carry_kernel<T>                what the next block's outputs still need of both
//
// A workgroup owns kSincBlockOut consecutive outputs of one row.  It copies the unit filter g (sinc(tau) * kaiser(tau / Z) at
// kSincTable(Z) + 1 equally spaced points of [0, Z], built by the host in fp64) into LDS once, then walks the inputs its outputs
// read, [floor(p_first - H), ceil(p_last + H)] cut to the row, in stretches of kSincStage samples staged in LDS (int16 widened
// as it is staged; outside the row the sum has no terms, which is what zeros there would add).  A thread owns kSincPerThread
// outputs, 256 apart, so that neighbouring lanes read neighbouring inputs and store neighbouring outputs.  Per tap: two LDS reads of g, one of x, no transcendental --
//   t = float(floor(p) - k) + float(p - floor(p))      one rounding: the relative error of t is 2^-24 at every distance
//   u = min(|t| * (N / H), N);  j = int(u);  c = g[j] + (u - j) * (g[j + 1] - g[j]);  acc += x[k] * c        k ascending
// and out = s * acc.  p = i * rate_in / rate_out is fp64 from i for every output, so an output's bits depend on its own row,
// its index and the parameters alone: not on the channel count, the strides, the workgroup it fell into or the run.
//
// gfx950 only.  wave = 64.  Compiled with -ffp-contract=off (see the Makefile): the two forms share their bits by construction.

#include "kernels.hpp"
#include "sinc_stream.hpp"
#include "sinc_taps.hpp"

namespace sd {

namespace {

// (sinc_sample, the LDS layout, SINC_WAVES_PER_SIMD and sinc_taps -- both kernels' arithmetic -- are in sinc_taps.hpp, shared with the
// packed recordings' load)

template <typename T>
__global__ void __launch_bounds__(256) SINC_WAVES_PER_SIMD
convert_rate_sinc_kernel(const T *__restrict__ in, int64_t n_in, int64_t in_stride, float *__restrict__ out, int64_t n_out,
                         int64_t out_stride, double rate_in, double rate_out, double H, float scale, float idx_scale,
                         const float *__restrict__ table, int N)
{
    float *g = reinterpret_cast<float *>(sinc_smem);         // [N + 4]
    float *xs = g + (N + 4);                                 // [kSincStage]
    const int tid = threadIdx.x;
    const T *row = in + (int64_t)blockIdx.y * in_stride;
    float *dst = out + (int64_t)blockIdx.y * out_stride;
    const int64_t i0 = (int64_t)blockIdx.x * kSincBlockOut;
    const int64_t i_last = min(i0 + (int64_t)kSincBlockOut, n_out) - 1;      // >= i0: the grid covers n_out exactly

    for (int e = tid; e < (N + 4) / 4; e += 256)             // (the table's buffer is 16-byte aligned and N % 4 == 0)
        reinterpret_cast<float4 *>(g)[e] = reinterpret_cast<const float4 *>(table)[e];

    // this thread's outputs: position, first and last tap (cut to the row), running sum
    int64_t pf[kSincPerThread], k_lo[kSincPerThread], k_hi[kSincPerThread];
    float frac[kSincPerThread], acc[kSincPerThread];
#pragma unroll
    for (int r = 0; r < kSincPerThread; r++) {
        const int64_t i = i0 + tid + (int64_t)r * 256;
        const double p = (double)i * rate_in / rate_out;
        const double fl = floor(p);
        pf[r] = (int64_t)fl;
        frac[r] = (float)(p - fl);
        k_lo[r] = max((int64_t)ceil(p - H), (int64_t)0);
        k_hi[r] = i <= i_last ? min((int64_t)floor(p + H), n_in - 1) : (int64_t)-1;      // past the row's end: no tap
        acc[r] = 0.0f;
    }
    // the inputs the workgroup reads (positions grow with i: the first output reaches furthest back, the last furthest on)
    const int64_t lo = max((int64_t)floor((double)i0 * rate_in / rate_out - H), (int64_t)0);
    const int64_t hi = min((int64_t)ceil((double)i_last * rate_in / rate_out + H), n_in - 1);
    const float n_f = (float)N;

    for (int64_t base = lo; base <= hi; base += kSincStage) {
        __syncthreads();                                     // the table is in; the stretch before this one is read out
        const int64_t end = min(base + kSincStage - 1, hi);                              // 0 <= base <= end <= n_in - 1
        for (int e = tid; e <= (int)(end - base); e += 256) xs[e] = sinc_sample<T>(row[base + e]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kSincPerThread; r++) {
            const int64_t ka = max(k_lo[r], base), kb = min(k_hi[r], end);
            if (ka > kb) continue;
            // |floor(p) - ka| <= H + 1 < 2^17
            acc[r] = sinc_taps(N, (int)(ka - base), (int)(kb - ka) + 1, (int)(pf[r] - ka), frac[r], idx_scale, n_f, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kSincPerThread; r++) {
        const int64_t i = i0 + tid + (int64_t)r * 256;
        if (i <= i_last) dst[i] = scale * acc[r];
    }
}

// The streaming form (the streaming sinc convention of include/syldet.h): the outputs m0 .. m0 + n_emit - 1 of a stream that had
// n_before samples before this push, written to out[0 .. n_emit).  Inputs are addressed absolutely: sample k < n_before comes
// from the handle's history row (fp32, the last min(n_before, L) samples), sample k >= n_before from the pushed row; the row ends
// at n_end (n_before + the push's length; a flush: n_before, and `in` is never read).  sinc_stream.hpp holds the addressing.
template <typename T>
__global__ void __launch_bounds__(256) SINC_WAVES_PER_SIMD
convert_rate_sinc_stream_kernel(const float *__restrict__ hist, int64_t L, const T *__restrict__ in, int64_t in_stride,
                                int64_t n_before, int64_t n_end, float *__restrict__ out, int64_t out_stride, int64_t m0,
                                int64_t n_emit, double rate_in, double rate_out, double H, float scale, float idx_scale,
                                const float *__restrict__ table, int N)
{
    float *g = reinterpret_cast<float *>(sinc_smem);         // [N + 4]
    float *xs = g + (N + 4);                                 // [kSincStage]
    const int tid = threadIdx.x;
    const float *hrow = hist + (int64_t)blockIdx.y * L;
    const T *row = in + (int64_t)blockIdx.y * in_stride;
    float *dst = out + (int64_t)blockIdx.y * out_stride;
    const int64_t i0 = m0 + (int64_t)blockIdx.x * kSincBlockOut;
    const int64_t i_last = min(i0 + (int64_t)kSincBlockOut, m0 + n_emit) - 1;            // >= i0: the grid covers n_emit exactly

    for (int e = tid; e < (N + 4) / 4; e += 256)
        reinterpret_cast<float4 *>(g)[e] = reinterpret_cast<const float4 *>(table)[e];

    int64_t pf[kSincPerThread], k_lo[kSincPerThread], k_hi[kSincPerThread];
    float frac[kSincPerThread], acc[kSincPerThread];
#pragma unroll
    for (int r = 0; r < kSincPerThread; r++) {
        const int64_t i = i0 + tid + (int64_t)r * 256;
        const double p = (double)i * rate_in / rate_out;
        const double fl = floor(p);
        pf[r] = (int64_t)fl;
        frac[r] = (float)(p - fl);
        k_lo[r] = max((int64_t)ceil(p - H), (int64_t)0);
        k_hi[r] = i <= i_last ? min((int64_t)floor(p + H), n_end - 1) : (int64_t)-1;
        acc[r] = 0.0f;
    }
    const int64_t lo = sinc_stream_stage_lo(i0, n_before, L, rate_in, rate_out, H);      // never before the history's first sample
    const int64_t hi = sinc_stream_stage_hi(i_last, n_end, rate_in, rate_out, H);
    const float n_f = (float)N;

    for (int64_t base = lo; base <= hi; base += kSincStage) {
        __syncthreads();
        const int64_t end = min(base + kSincStage - 1, hi);  // hist_first <= base <= end <= n_end - 1
        for (int e = tid; e <= (int)(end - base); e += 256) {
            const int64_t k = base + e;
            xs[e] = sinc_stream_in_history(k, n_before) ? hrow[sinc_stream_hist_offset(k, n_before, L)]
                                                        : sinc_sample<T>(row[sinc_stream_push_offset(k, n_before)]);
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kSincPerThread; r++) {
            const int64_t ka = max(k_lo[r], base), kb = min(k_hi[r], end);
            if (ka > kb) continue;
            acc[r] = sinc_taps(N, (int)(ka - base), (int)(kb - ka) + 1, (int)(pf[r] - ka), frac[r], idx_scale, n_f, acc[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < kSincPerThread; r++) {
        const int64_t i = i0 + tid + (int64_t)r * 256;
        if (i <= i_last) dst[i - m0] = scale * acc[r];
    }
}

// The next history, into the OTHER buffer (the kernel above reads the current one in the same push): the last min(n_before + n, L)
// samples of history ++ push, the push widened as it is kept.
template <typename T>
__global__ void __launch_bounds__(256)
sinc_carry_kernel(const float *__restrict__ hist, float *__restrict__ next, int64_t L, const T *__restrict__ in, int64_t in_stride,
                  int64_t n_before, int64_t n)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= sinc_stream_hist_len(n_before + n, L)) return;
    const int64_t k = sinc_stream_carry_sample(j, n_before, n, L);                       // hist_first(n_before) <= k < n_before + n
    const float v = sinc_stream_in_history(k, n_before)
                        ? hist[(int64_t)blockIdx.y * L + sinc_stream_hist_offset(k, n_before, L)]
                        : sinc_sample<T>(in[(int64_t)blockIdx.y * in_stride + sinc_stream_push_offset(k, n_before)]);
    next[(int64_t)blockIdx.y * L + j] = v;
}

template <typename T>
hipError_t launch_sinc_stream(const float *hist, float *next, int64_t L, const T *in, int64_t n_in, int64_t in_stride,
                              int64_t n_before, float *out, int64_t out_stride, int64_t m0, int64_t n_emit, int C, double rate_in,
                              double rate_out, double H, float scale, const float *table, int N, hipStream_t stream)
{
    if (C <= 0) return hipSuccess;
    if (n_emit > 0) {
        auto kern = convert_rate_sinc_stream_kernel<T>;
        const int lds = (N + 4 + kSincStage) * (int)sizeof(float);
        hipError_t st = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (st != hipSuccess) return st;
        dim3 grid((unsigned)((n_emit + kSincBlockOut - 1) / kSincBlockOut), (unsigned)C);
        hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)lds, stream, hist, L, in, in_stride, n_before, n_before + n_in, out,
                           out_stride, m0, n_emit, rate_in, rate_out, H, scale, (float)((double)N / H), table, N);
        st = hipGetLastError();
        if (st != hipSuccess) return st;
    }
    if (n_in > 0) {
        const int64_t len = sinc_stream_hist_len(n_before + n_in, L);
        dim3 grid((unsigned)((len + 255) / 256), (unsigned)C);
        hipLaunchKernelGGL(sinc_carry_kernel<T>, grid, dim3(256), 0, stream, hist, next, L, in, in_stride, n_before, n_in);
        return hipGetLastError();
    }
    return hipSuccess;
}

template <typename T>
hipError_t launch_sinc(const T *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out, int64_t out_stride, int C,
                       double rate_in, double rate_out, double H, float scale, const float *table, int N, hipStream_t stream)
{
    if (n_out <= 0 || C <= 0) return hipSuccess;
    auto kern = convert_rate_sinc_kernel<T>;
    const int lds = (N + 4 + kSincStage) * (int)sizeof(float);
    // 80 KB (Z <= 32: two workgroups a CU) or 144 KB (one); the attribute is per device, so it is set on every launch
    hipError_t st = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (st != hipSuccess) return st;
    dim3 grid((unsigned)((n_out + kSincBlockOut - 1) / kSincBlockOut), (unsigned)C);
    hipLaunchKernelGGL(kern, grid, dim3(256), (size_t)lds, stream, in, n_in, in_stride, out, n_out, out_stride, rate_in, rate_out,
                       H, scale, (float)((double)N / H), table, N);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_convert_rate_sinc(const float *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out,
                                    int64_t out_stride, int C, double rate_in, double rate_out, double H, float scale,
                                    const float *table, int N, hipStream_t stream)
{
    return launch_sinc<float>(in, n_in, in_stride, out, n_out, out_stride, C, rate_in, rate_out, H, scale, table, N, stream);
}

hipError_t launch_convert_rate_sinc_s16(const int16_t *in, int64_t n_in, int64_t in_stride, float *out, int64_t n_out,
                                        int64_t out_stride, int C, double rate_in, double rate_out, double H, float scale,
                                        const float *table, int N, hipStream_t stream)
{
    return launch_sinc<int16_t>(in, n_in, in_stride, out, n_out, out_stride, C, rate_in, rate_out, H, scale, table, N, stream);
}

hipError_t launch_sinc_stream_push(const float *hist, float *next, int64_t L, const float *in, int64_t n_in, int64_t in_stride,
                                   int64_t n_before, float *out, int64_t out_stride, int64_t m0, int64_t n_emit, int C,
                                   double rate_in, double rate_out, double H, float scale, const float *table, int N,
                                   hipStream_t stream)
{
    return launch_sinc_stream<float>(hist, next, L, in, n_in, in_stride, n_before, out, out_stride, m0, n_emit, C, rate_in, rate_out,
                                     H, scale, table, N, stream);
}

hipError_t launch_sinc_stream_push_s16(const float *hist, float *next, int64_t L, const int16_t *in, int64_t n_in, int64_t in_stride,
                                       int64_t n_before, float *out, int64_t out_stride, int64_t m0, int64_t n_emit, int C,
                                       double rate_in, double rate_out, double H, float scale, const float *table, int N,
                                       hipStream_t stream)
{
    return launch_sinc_stream<int16_t>(hist, next, L, in, n_in, in_stride, n_before, out, out_stride, m0, n_emit, C, rate_in, rate_out,
                                       H, scale, table, N, stream);
}

}  // namespace sd
