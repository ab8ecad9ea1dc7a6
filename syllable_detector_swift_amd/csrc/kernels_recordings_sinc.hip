// kernels_recordings_sinc.hip -- packed recordings at other rates (syldet_recordings_load_sinc_device* of include/syldet.h): every
// recording of a plan converted to the network's rate straight into its place in the bank's rows, in one launch.  The reference's
// tool has AVFoundation deliver every file at the network's rate (SyllableDetector.swift:19-23, TrackDetector.swift:35) and runs
// the files one after another (SyllableDetectorCLI/main.swift:63-130).
//
//   recordings_load_sinc_kernel<float>     fp32 sources
//   recordings_load_sinc_kernel<int16_t>   16-bit PCM sources (x means float(x) * 2^-15), widened as they are staged
//   recordings_load_sinc_kernel<uint8_t>   the files' own bytes (syldet_recordings_load_sinc_pcm_device): src_offset and src_step
//                                          count bytes, and a sample is the slot's format's value (pcm_values.hpp) -- the slot is
//                                          the workgroup's, so the format decides a scalar branch
//
// grid (workgroups of the fullest row, C).  Row c's slots own consecutive workgroups of the row, kSincBlockOut row positions of a
// slot's span [offset, span_end) each; the workgroup finds its slot by a binary search of the row's prefix table with its block
// index (uniform: scalar loads), so that the tables are K + C words whatever the recordings' lengths.  For the positions that are
// outputs of a recording at another rate it is convert_rate_sinc_kernel (kernels_sinc.hip) on that recording alone: the same
// table in LDS, the same stretches of kSincStage inputs (read with the slot's step: the call is also the de-interleave), the same
// fp64 position p = i * rate_in / rate_out with i counted from the recording's start, the same sinc_taps (sinc_taps.hpp) -- the
// bits of syldet_convert_rate_sinc_device*.  A recording at the network's rate is copied (widened), not low-passed; every other
// position of the span, and every position of a row without a recording, is +0.  Stores are 4 bytes a lane, neighbouring lanes
// neighbouring positions: row offsets are multiples of hop, which may be odd.
//
// gfx950 only.  wave = 64.  Compiled with -ffp-contract=off, as kernels_sinc.hip is (see the Makefile).

#include "kernels.hpp"
#include "pcm_values.hpp"
#include "sinc_taps.hpp"

namespace sd {

namespace {

// the sample at in[at] (fp32, int16), or the `format` value at byte `at` of in
template <typename T>
__device__ __forceinline__ float rec_sample(const T *__restrict__ in, int64_t at, int) { return sinc_sample<T>(in[at]); }
template <>
__device__ __forceinline__ float rec_sample<uint8_t>(const uint8_t *__restrict__ in, int64_t at, int format) { return pcm_value(format, in + at); }

template <typename T>
__global__ void __launch_bounds__(256) SINC_WAVES_PER_SIMD
recordings_load_sinc_kernel(RecSincDesc d, const T *__restrict__ src, double rate_out, const float *__restrict__ table, int N,
                            float *__restrict__ rows, int64_t stride)
{
    float *g = reinterpret_cast<float *>(sinc_smem);         // [N + 4]
    float *xs = g + (N + 4);                                 // [kSincStage]
    const int tid = threadIdx.x;
    const int c = blockIdx.y;
    const int b = blockIdx.x;
    float *row = rows + (int64_t)c * stride;
    const int sb = d.row_begin[c], sn = d.row_begin[c + 1] - sb;
    if (sn == 0) {                                           // a row without a recording: +0
        const int64_t q0 = (int64_t)b * kSincBlockOut;
#pragma unroll
        for (int r = 0; r < kSincPerThread; r++) {
            const int64_t q = q0 + tid + (int64_t)r * 256;
            if (q < d.row_samples) row[q] = 0.0f;
        }
        return;
    }
    const int32_t *wg = d.wg_begin + sb + c;                 // [sn + 1]
    if (b >= wg[sn]) return;                                 // (the grid is the fullest row's)
    // the last slot whose first workgroup is at or before b: it owns b (a slot without a workgroup shares its successor's start)
    int lo = 0, hi = sn - 1;                                 // wg[lo] <= b < wg[hi + 1]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (wg[mid] <= b) lo = mid;
        else hi = mid - 1;
    }
    lo = __builtin_amdgcn_readfirstlane(lo);
    const RecSincDev s = d.slots[sb + lo];
    const int64_t i0 = (int64_t)(b - wg[lo]) * kSincBlockOut;                // counted from the recording's start
    const int64_t span = s.span_end - s.offset;                              // > i0
    const int64_t n_out = s.n_out, n_in = s.n_in;
    const int64_t step = s.src_step;
    const int format = s.format;
    const T *in = src + s.src_offset;
    float *dst = row + s.offset;

    if (s.copy || i0 >= n_out) {                             // at the network's rate, or behind the recording's last output
#pragma unroll
        for (int r = 0; r < kSincPerThread; r++) {
            const int64_t i = i0 + tid + (int64_t)r * 256;
            if (i < span) dst[i] = i < n_out ? rec_sample<T>(in, i * step, format) : 0.0f;      // (copy: n_out <= n_in)
        }
        return;
    }

    // from here on convert_rate_sinc_kernel on the recording alone, statement for statement
    const double rate_in = s.rate_in, H = s.H;
    const float scale = s.scale, idx_scale = s.idx_scale;
    const int64_t i_last = min(i0 + (int64_t)kSincBlockOut, n_out) - 1;      // >= i0

    for (int e = tid; e < (N + 4) / 4; e += 256)             // (the table's buffer is 16-byte aligned and N % 4 == 0)
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
        k_hi[r] = i <= i_last ? min((int64_t)floor(p + H), n_in - 1) : (int64_t)-1;      // past the recording's end: no tap
        acc[r] = 0.0f;
    }
    const int64_t in_lo = max((int64_t)floor((double)i0 * rate_in / rate_out - H), (int64_t)0);
    const int64_t in_hi = min((int64_t)ceil((double)i_last * rate_in / rate_out + H), n_in - 1);
    const float n_f = (float)N;

    for (int64_t base = in_lo; base <= in_hi; base += kSincStage) {
        __syncthreads();                                     // the table is in; the stretch before this one is read out
        const int64_t end = min(base + kSincStage - 1, in_hi);                           // 0 <= base <= end <= n_in - 1
        for (int e = tid; e <= (int)(end - base); e += 256) xs[e] = rec_sample<T>(in, (base + e) * step, format);
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
        else if (i < span) dst[i] = 0.0f;                    // the pad behind the recording
    }
}

template <typename T>
hipError_t load_sinc_as(const RecSincDesc &d, const void *src, double rate_out, const float *table, int N, float *rows, int64_t stride,
                        int C, hipStream_t stream)
{
    auto kern = recordings_load_sinc_kernel<T>;
    const int lds = (N + 4 + kSincStage) * (int)sizeof(float);
    // 80 KB (Z <= 32) or 144 KB, as the whole-recording converter; the attribute is per device, so it is set on every launch
    hipError_t st = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if (st != hipSuccess) return st;
    hipLaunchKernelGGL(kern, dim3((unsigned)d.grid_x, (unsigned)C), dim3(256), (size_t)lds, stream, d, (const T *)src, rate_out, table, N,
                       rows, stride);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_recordings_load_sinc(const RecSincDesc &d, const void *src, bool s16, double rate_out, const float *table, int N,
                                       float *rows, int64_t stride, int C, hipStream_t stream)
{
    if (C <= 0 || d.grid_x <= 0) return hipSuccess;
    return s16 ? load_sinc_as<int16_t>(d, src, rate_out, table, N, rows, stride, C, stream)
               : load_sinc_as<float>(d, src, rate_out, table, N, rows, stride, C, stream);
}

hipError_t launch_recordings_load_sinc_pcm(const RecSincDesc &d, const void *src, double rate_out, const float *table, int N, float *rows,
                                           int64_t stride, int C, hipStream_t stream)
{
    if (C <= 0 || d.grid_x <= 0) return hipSuccess;
    return load_sinc_as<uint8_t>(d, src, rate_out, table, N, rows, stride, C, stream);
}

}  // namespace sd
