// kernels_recordings_levels.hip -- the two level meters of packed recordings (syldet_recordings_levels_device*,
// syldet_recordings_output_levels_device of include/syldet.h): every recording of a packed bank gets the readings it would have
// had alone (kernels_levels.hip), recording k's at elements [reading_first[k], reading_first[k + 1]) of one flat table, in a fixed
// number of launches whatever K is.
//
//   recordings_meter_zero_kernel      the table <- +0, where a reading may cross workgroups; syldet_timings lists it as
//                                     "recordings_levels_zero_kernel"
//   recordings_meter_in_kernel<T>     packed rows [C][stride], fp32 or int16 -> every recording's mean squares, fp64;
//                                     "recordings_levels_in_kernel" (the symbols have other names because the build's ISA check of
//                                     kernels_levels.hip finds that file by the text of its kernel's name)
//   recordings_meter_out_kernel       outputs [C][row_evals][n_out] -> every recording's output levels, fp32;
//                                     "recordings_levels_out_kernel"
//
// The values are those of the one-recording kernels (levels_values.hpp states each once); what differs is where a recording
// begins.  Buffer b of a recording of n samples at row offset o is the row positions [o + b L, o + min((b + 1) L, n)): the tree's
// leaves, the lane groups and the buffer count B = ceil(n / L) are all counted from o, a short last buffer is masked at n (the next
// recording may begin within L samples of it: nothing behind n is ever read), and P is clamped to the recording's own B.
//
// The input meter is balanced by ROWS, not by recordings (lengths differ by orders of magnitude): workgroup (t, c) takes 32 KiB of
// row c -- one of the load's tiles of kRecTile samples for fp32 rows, two for int16 rows -- finds its first slot in the load's
// tile_first table and walks the slots that cross its span.  Of each slot it OWNS the buffers whose first sample lies in the span: every buffer has exactly one owner, and an owner
// reads at most L - 1 samples behind its span. A reading whose buffers all have one owner is stored plainly.  A reading that
// crosses workgroups is made with one atomic an owner: the table is +0 beforehand, a mean square that is not NaN is a non-negative
// double, whose bits order as an unsigned 64-bit integer, so an atomic max on the bits leaves the greatest of them whatever the
// order; the owner of the reading's FIRST buffer contributes the canonical quiet NaN (above +inf in that order) where that
// buffer's value is NaN, and nobody else contributes a NaN -- StatMax exactly, deterministic, no second pass, and no workgroup
// waits for another.
//
// Compiled like kernels_levels.hip: -ffp-contract=off, no fast-math flag (see the Makefile).
//
// gfx950 only.  wave = 64.  Every value is written with ordinary vector stores and vector atomics.

#include "kernels.hpp"
#include "levels_values.hpp"

namespace sd {

namespace {

constexpr int kBlock = 256;
constexpr unsigned long long kQuietNaN = 0x7ff8000000000000ull;

// the 16 bytes of the whole group at p, by the widest loads its address allows (`align`: the address modulo 16, the same for
// every group of a slot)
template <typename T>
__device__ __forceinline__ u32x4 load_group(const T *p, unsigned align)
{
    if (align == 0) return __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
    if (align == 8) {
        const uint2 a = *reinterpret_cast<const uint2 *>(p), b = *(reinterpret_cast<const uint2 *>(p) + 1);
        return u32x4{a.x, a.y, b.x, b.y};
    }
    if ((align & 3u) == 0) {
        const unsigned *w = reinterpret_cast<const unsigned *>(p);
        return u32x4{w[0], w[1], w[2], w[3]};
    }
    return load_each(p, 0, 16 / (int)sizeof(T));
}

}  // namespace

__global__ void __launch_bounds__(kBlock)
recordings_meter_zero_kernel(double *__restrict__ out, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = 0.0;
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
recordings_meter_in_kernel(RecLevelsDesc d, const T *__restrict__ rows, int64_t stride, int L, int64_t P, double *__restrict__ out)
{
    constexpr int G = 16 / (int)sizeof(T);             // samples per 16-byte group
    constexpr int kTiles = 4 / (int)sizeof(T);         // tiles a workgroup: 32 KiB of the row either way, as levels_in_kernel
    constexpr int kSpan = kRecTile * kTiles;           // (with one tile of int16 -- 16 KiB, four loads a lane -- the meter took 1.5x the plain one's time)
    constexpr int kPasses = kSpan / (kBlock * G);      // 16-byte loads a lane has in flight: a slot's part of the span in one sweep
    constexpr int kReach = 64 * G;                     // samples of one wave in one pass
    __shared__ float sums[kSpan / 8];                  // one per min(L, kReach) samples
    const int c = blockIdx.y, tid = threadIdx.x;
    const int64_t p0 = (int64_t)blockIdx.x * kSpan, p1 = min(p0 + (int64_t)kSpan, d.load.row_samples);
    const int lpb = L / G;                             // lanes a buffer (1: a lane holds a whole buffer of 8 int16)
    const int lead = min(lpb, 64), lead_shift = __ffs(lead) - 1;
    const int se = d.load.row_begin[c + 1];
    for (int s = d.load.tile_first[(int64_t)c * d.load.tiles + (int64_t)blockIdx.x * kTiles]; s < se; s++) {
        const RecSlotDev sl = d.load.slots[s];
        if (sl.offset >= p1) break;
        const int64_t n = sl.n_samples;
        const int64_t B = (n + L - 1) / L;
        // the owned buffers [bA, bB): their first samples o + b L lie in [p0, p1)
        const int64_t bA = sl.offset >= p0 ? 0 : (p0 - sl.offset + L - 1) / L, bB = min((p1 - sl.offset + L - 1) / L, B);
        if (bA >= bB) continue;                        // (a pad, a recording without samples, or one whose buffers begin elsewhere)
        const T *rec = rows + (int64_t)c * stride + sl.offset;
        const unsigned align = (unsigned)(reinterpret_cast<uintptr_t>(rec) & 15u);
        const int64_t base = bA * L, end = min(bB * L, n);   // at most kSpan samples: kSpan / L buffers begin in the span

        u32x4 raw[kPasses];
#pragma unroll
        for (int j = 0; j < kPasses; j++) {
            const int64_t i = base + (int64_t)(j * kBlock + tid) * G;
            if (i + G <= end) raw[j] = load_group(rec + i, align);
            else if (i < end) raw[j] = load_each(rec, i, (int)(end - i));
            else raw[j] = u32x4{0u, 0u, 0u, 0u};
        }
        __syncthreads();                               // (the slot before has been read out of sums)
#pragma unroll
        for (int j = 0; j < kPasses; j++) {
            const float p = lanes_sum<T>(raw[j], lpb);
            if ((tid & (lead - 1)) == 0) sums[(j * kBlock + tid) >> lead_shift] = p;
        }
        __syncthreads();
        const int r = lds_tree<kSpan, kReach>(sums, L, tid);
        // Double(sum) / Double(length): the recording's last buffer divides by its own length
        auto value = [&](int64_t b) {
            const int64_t len = b == B - 1 ? n - b * L : (int64_t)L;
            return (double)sums[(int)(b - bA) * r] / (double)len;
        };
        const int64_t Pk = min(P, B);                  // (one reading either way; keeps m P inside 64 bits)
        const int64_t m0 = bA / Pk, m1 = (bB - 1) / Pk;
        const int nr = (int)(m1 - m0 + 1);
        double *dst = out + d.slot_first[s];
        // `best`: the greatest value of [lo, hi) that is not NaN (-1: none)
        auto emit = [&](int64_t m, int64_t lo, double best) {
            const bool has_first = lo == m * Pk;
            const double first = has_first ? value(lo) : 0.0;
            if (has_first && min((m + 1) * Pk, B) <= bB) {
                dst[m] = first != first ? first : best;
            } else {
                unsigned long long *word = reinterpret_cast<unsigned long long *>(dst + m);
                if (first != first) atomicMax(word, kQuietNaN);
                else if (best >= 0.0) atomicMax(word, (unsigned long long)__double_as_longlong(best));
            }
        };
        if (Pk < 16) {
            // short readings: a lane each
            for (int i = tid; i < nr; i += kBlock) {
                const int64_t m = m0 + i, lo = max(m * Pk, bA), hi = min((m + 1) * Pk, bB);
                emit(m, lo, best_of_lane(lo, hi, value));
            }
        } else {
            // long readings: a wave each
            const int lane = tid & 63;
            for (int i = tid >> 6; i < nr; i += 4) {
                const int64_t m = m0 + i, lo = max(m * Pk, bA), hi = min((m + 1) * Pk, bB);
                const double best = best_of_wave(lo, hi, lane, value);
                if (lane == 0) emit(m, lo, best);
            }
        }
    }
}

// Reading g of the flat table: recording k by a search in the prefix, then levels_out_kernel's reading m = g - reading_first[k] of
// that recording alone, its evaluation e at row evaluation first_eval + e.  WAVE: a wave a reading, else a lane.
template <bool WAVE>
__global__ void __launch_bounds__(kBlock)
recordings_meter_out_kernel(RecLevelsDesc d, const float *__restrict__ outputs, int n_out, int k_out, int L, int64_t P, int64_t need,
                            int64_t hop, int T, float *__restrict__ levels)
{
    const int lane = WAVE ? (int)(threadIdx.x & 63) : 0;
    const int64_t g = WAVE ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= d.n_readings) return;
    // the last k with reading_first[k] <= g (recordings without a reading share their successor's entry and are passed over)
    int lo = 0, hi = d.K;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d.reading_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    const int k = lo;
    const RecEventDev rec = d.events[k];
    const int64_t n = d.n_samples[k], B = (n + L - 1) / L, PL = min(P, B) * L;
    const float *row = outputs + ((int64_t)rec.row * d.row_evals + rec.first_eval) * n_out + k_out;
    const float result = levels_out_value<WAVE>(row, rec.n_evals, n_out, g - d.reading_first[k], n, PL, need, hop, T, lane);
    if (lane == 0) levels[g] = result;
}

hipError_t launch_recordings_levels_zero(double *mean_square, int64_t n_readings, hipStream_t stream)
{
    if (n_readings <= 0) return hipSuccess;
    const int64_t blocks = (n_readings + kBlock - 1) / kBlock;
    if (!mean_square || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recordings_meter_zero_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, stream, mean_square, n_readings);
    return hipGetLastError();
}

hipError_t launch_recordings_levels_in(const RecLevelsDesc &d, int C, const void *rows, bool s16, int64_t stride, int L, int64_t P,
                                       double *mean_square, hipStream_t stream)
{
    if (C <= 0 || d.K <= 0 || d.load.tiles <= 0 || d.n_readings <= 0) return hipSuccess;
    if (L < 8 || L > 4096 || (L & (L - 1)) != 0 || P < 1 || stride < d.load.row_samples || C > 65535 || !rows || !mean_square ||
        (reinterpret_cast<uintptr_t>(rows) & (s16 ? 1u : 3u)) != 0)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)(s16 ? (d.load.tiles + 1) / 2 : d.load.tiles), (unsigned)C);   // (kTiles of the kernel)
    if (s16)
        hipLaunchKernelGGL(recordings_meter_in_kernel<int16_t>, grid, dim3(kBlock), 0, stream, d, (const int16_t *)rows, stride, L, P, mean_square);
    else
        hipLaunchKernelGGL(recordings_meter_in_kernel<float>, grid, dim3(kBlock), 0, stream, d, (const float *)rows, stride, L, P, mean_square);
    return hipGetLastError();
}

hipError_t launch_recordings_levels_out(const RecLevelsDesc &d, int C, const float *outputs, int n_out, int k, int L, int64_t P, int64_t need,
                                        int64_t hop, int T, float *levels, hipStream_t stream)
{
    if (C <= 0 || d.K <= 0 || d.n_readings <= 0) return hipSuccess;
    if (L < 8 || L > 4096 || (L & (L - 1)) != 0 || P < 1 || n_out < 1 || k < 0 || k >= n_out || hop < 1 || T < 1 || !levels ||
        (d.row_evals > 0 && !outputs))
        return hipErrorInvalidValue;
    // a wave a reading where readings hold more than a few evaluations (launch_levels_out's rule, over the whole bank)
    const bool wave = (int64_t)C * d.row_evals / d.n_readings > 8;
    const int64_t blocks = wave ? (d.n_readings + 3) / 4 : (d.n_readings + kBlock - 1) / kBlock;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (wave)
        hipLaunchKernelGGL(recordings_meter_out_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, d, outputs, n_out, k, L, P, need,
                           hop, T, levels);
    else
        hipLaunchKernelGGL(recordings_meter_out_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), 0, stream, d, outputs, n_out, k, L, P, need,
                           hop, T, levels);
    return hipGetLastError();
}

}  // namespace sd
