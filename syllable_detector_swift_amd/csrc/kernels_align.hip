// kernels_align.hip -- event-aligned windows (syldet_align_device, syldet_align_stats_device of include/syldet.h): the units of a
// source around every event, one window an event, and the stack statistics of groups of windows in a fixed tree.
//
//   align_windows_kernel   A window is one contiguous span of the source copied to one contiguous span of the destination, with
//                  `fill` on either side (align_span.hpp: the clipped span, the text the host runs).  A team of lanes takes
//                  consecutive windows: a wave where a window is short (four windows each, so that the search for the first
//                  window's detector is made once for four), the workgroup where it is long.  Everything of a window that is not
//                  a lane's own -- its detector, the detector's row, base and units, the event, the span -- is the team's and is
//                  computed on uniform values (scalar registers).  The destination is written 16 bytes a lane in groups aligned
//                  to the destination's address, its head and tail element by element; a group that lies inside the present
//                  span is loaded 16 bytes from its 4-byte-aligned source address, any other group element by element with the
//                  fill selected in.  Every element of the destination is written exactly once; no LDS, no barrier.
//   align_stats_kernel     A thread owns a position p of one block of at most 256 events of a group and walks the block's windows in
//                  order: count, sum and sum of squares (fp64, from +0.0) of the elements that are present by the spans the
//                  windows kernel left.  Consecutive threads read consecutive p.
//   align_combine_kernel   adds a group's block results in block order, from +0.0.
//
// gfx950 only: wave = 64 lanes.  Plain HIP C++, vector loads and stores.

#include "align_span.hpp"
#include "kernels.hpp"

namespace sd {

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWavePer = 4;                  // consecutive windows a wave takes
constexpr int kShort = 1024;                 // elements: windows up to here go to waves, longer ones to workgroups

typedef float f4 __attribute__((ext_vector_type(4)));

// 16 bytes from a 4-byte-aligned address
__device__ __forceinline__ f4 load4_unaligned(const float *__restrict__ p)
{
    f4 v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}

template <int TEAM>
__global__ void __launch_bounds__(kThreads)
align_windows_kernel(AlignDesc d, const float *__restrict__ src, int64_t n_units, int64_t row_stride, const int64_t *__restrict__ events,
                     int64_t event_stride, int64_t N, int per, float fill, float *__restrict__ windows)
{
    constexpr int teams = kThreads / TEAM;
    const int team = TEAM == kThreads ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x / TEAM);
    const int lane = (int)threadIdx.x % TEAM;
    const int64_t w0 = ((int64_t)blockIdx.x * teams + team) * per;
    if (w0 >= N) return;
    const int64_t w1 = w0 + per < N ? w0 + per : N;
    const int width = d.width;
    const int L = (int)((d.before + d.after + 1) * width);                // <= 2^20
    // the detector of window w0: the first whose events end behind it (N = event_begin[D] > w0: there is one)
    int lo = 0, hi = d.D - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (d.event_begin[mid + 1] > w0) hi = mid;
        else lo = mid + 1;
    }
    int det = lo;
    int64_t begin = d.event_begin[det], end = d.event_begin[det + 1];
    for (int64_t w = w0; w < w1; w++) {
        while (w >= end) {                                                // (detectors without events are stepped over)
            det++;
            begin = end;
            end = d.event_begin[det + 1];
        }
        int64_t row = det, base = 0, U = n_units;
        if (d.dets) {
            const DetSpan e = d.dets[det];
            row = e.row;
            base = e.first;
            U = e.units;
        }
        const int64_t s = events[event_stride ? (int64_t)det * event_stride + (w - begin) : w];
        const AlignSpan sp = align_span(s, d.origin, d.step, d.before, d.after, U);
        const int p0 = (int)sp.first * width, p1 = p0 + (int)sp.count * width;     // the present elements of the window
        // element p of the window, p0 <= p < p1, is from[p]
        const float *__restrict__ from = src + row * row_stride + (base + sp.unit) * (int64_t)width - p0;
        float *__restrict__ dst = windows + w * (int64_t)L;
        if (lane == 0) d.spans[w] = make_int2(p0, p1 - p0);
        auto value = [&](int p) { return p >= p0 && p < p1 ? from[p] : fill; };
        int head = (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) >> 2);  // elements in front of the first 16-byte line
        head = head < L ? head : L;
        const int body = (L - head) >> 2, tail = L - head - 4 * body;
        if (lane < head) dst[lane] = value(lane);
        if (lane < tail) dst[head + 4 * body + lane] = value(head + 4 * body + lane);
        for (int g = lane; g < body; g += TEAM) {
            const int p = head + 4 * g;
            f4 v;
            if (p >= p0 && p + 4 <= p1) {
                v = load4_unaligned(from + p);                            // (global_load_dwordx4: the address need not be a multiple of 16)
            } else {
                v.x = value(p);
                v.y = value(p + 1);
                v.z = value(p + 2);
                v.w = value(p + 3);
            }
            *reinterpret_cast<f4 *>(dst + p) = v;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
align_stats_kernel(AlignStatsDesc d, const float *__restrict__ windows, int L, int chunks)
{
    const int64_t b = blockIdx.x / (unsigned)chunks;
    const int p = (int)(blockIdx.x % (unsigned)chunks) * kThreads + (int)threadIdx.x;
    const int g = d.block_group[b];
    const int64_t i0 = d.group_begin[g] + (b - d.block_begin[g]) * kAlignBlock;
    const int64_t stop = d.group_begin[g + 1], i1 = i0 + kAlignBlock < stop ? i0 + kAlignBlock : stop;
    int64_t n = 0;
    double sum = 0.0, sumsq = 0.0;
    for (int64_t i = i0; i < i1; i++) {
        const int64_t w = d.perm[i];
        const int2 sp = d.spans[w];
        if (p < L && (unsigned)(p - sp.x) < (unsigned)sp.y) {
            const double x = (double)windows[w * (int64_t)L + p];
            n++;
            sum = sum + x;
            sumsq = sumsq + x * x;                                        // (x * x is exact: an fp32 value's square has 48 bits)
        }
    }
    if (p < L) {
        d.part_count[b * (int64_t)L + p] = n;
        d.part_sum[b * (int64_t)L + p] = sum;
        d.part_sumsq[b * (int64_t)L + p] = sumsq;
    }
}

__global__ void __launch_bounds__(kThreads)
align_combine_kernel(AlignStatsDesc d, int L, int chunks, int64_t *__restrict__ count, double *__restrict__ sum, double *__restrict__ sumsq)
{
    const int g = (int)(blockIdx.x / (unsigned)chunks);
    const int p = (int)(blockIdx.x % (unsigned)chunks) * kThreads + (int)threadIdx.x;
    if (p >= L) return;
    int64_t n = 0;
    double s = 0.0, q = 0.0;
    for (int64_t b = d.block_begin[g]; b < d.block_begin[g + 1]; b++) {
        n += d.part_count[b * (int64_t)L + p];
        s = s + d.part_sum[b * (int64_t)L + p];
        q = q + d.part_sumsq[b * (int64_t)L + p];
    }
    count[g * (int64_t)L + p] = n;
    sum[g * (int64_t)L + p] = s;
    sumsq[g * (int64_t)L + p] = q;
}

template <int TEAM>
void launch_windows(const AlignDesc &d, const float *src, int64_t n_units, int64_t row_stride, const int64_t *events, int64_t event_stride,
                    int64_t N, int per, float fill, float *windows, hipStream_t stream)
{
    const int64_t per_block = (int64_t)(kThreads / TEAM) * per;
    const dim3 grid((unsigned)((N + per_block - 1) / per_block));
    hipLaunchKernelGGL(align_windows_kernel<TEAM>, grid, dim3(kThreads), 0, stream, d, src, n_units, row_stride, events, event_stride, N, per, fill,
                       windows);
}

}  // namespace

hipError_t launch_align_windows(const AlignDesc &d, const float *src, int64_t n_units, int64_t row_stride, const int64_t *events,
                                int64_t event_stride, int64_t N, float fill, float *windows, hipStream_t stream)
{
    if (N <= 0 || d.D <= 0) return hipSuccess;
    const int64_t L = (d.before + d.after + 1) * d.width;
    if (L <= kShort)
        launch_windows<kWave>(d, src, n_units, row_stride, events, event_stride, N, kWavePer, fill, windows, stream);
    else
        launch_windows<kThreads>(d, src, n_units, row_stride, events, event_stride, N, 1, fill, windows, stream);
    return hipGetLastError();
}

hipError_t launch_align_stats(const AlignStatsDesc &d, const float *windows, int L, hipStream_t stream)
{
    if (d.B <= 0 || L <= 0) return hipSuccess;
    const int chunks = (L + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(align_stats_kernel, dim3((unsigned)(d.B * chunks)), dim3(kThreads), 0, stream, d, windows, L, chunks);
    return hipGetLastError();
}

hipError_t launch_align_combine(const AlignStatsDesc &d, int L, int64_t *count, double *sum, double *sumsq, hipStream_t stream)
{
    if (d.G <= 0 || L <= 0) return hipSuccess;
    const int chunks = (L + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(align_combine_kernel, dim3((unsigned)((int64_t)d.G * chunks)), dim3(kThreads), 0, stream, d, L, chunks, count, sum, sumsq);
    return hipGetLastError();
}

}  // namespace sd
