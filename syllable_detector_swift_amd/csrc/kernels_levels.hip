// kernels_levels.hip -- the two level meters of a ProcessorBase row (SyllableDetector/Processor.swift:111-113, :138, :158-184;
// SummaryStat.swift's StatMax), for whole recordings: DESIGN.md 4.13.
//   levels_in_kernel<T>   planar rows [C][stride], fp32 or int16 (x * 2^-15): the mean square of every buffer of L samples, the
//                         StatMax of every reading of P buffers -> fp64 [C][M]
//   levels_fold_kernel    the readings that cross workgroups, from the partials the first kernel left
//   levels_out_kernel     the StatMax of output k over the evaluations each reading's buffers make available -> fp32 [C][M]
// A buffer's sum of squares is THIS LIBRARY'S sum_squares_tree (include/syldet.h): every square rounded to fp32, the squares added
// as a balanced binary tree in index order over next_pow2(n) slots, every addition rounded to fp32.  A lane holds the tree's lowest
// levels (the 16 bytes it loads), the lanes of a wave the next ones (exchanges over xor distances 1, 2, 4 ...: addition is
// commutative, so the butterfly is the tree), LDS the rest.  StatMax is written as comparisons: the first value as it is, a later
// one only if it is greater -- NaN first sticks, NaN later is ignored.
//
// gfx950 only.  wave = 64.

#include <algorithm>

#include "kernels.hpp"
#include "levels_values.hpp"

// a square, an addition: each rounds on its own -- this file is compiled with -ffp-contract=off (see the Makefile).  The value
// arithmetic itself is in levels_values.hpp, which the packed recordings' meters (kernels_recordings_levels.hip) share.

namespace sd {

namespace {

constexpr int kLevelsPasses = 8;                        // 16-byte loads a lane has in flight
constexpr int kLevelsSpanBytes = 256 * 16 * kLevelsPasses;   // bytes of one channel's row per workgroup: 8192 fp32 / 16384 int16
                                                        // samples, whole buffers for every L <= 4096

}  // namespace

// Workgroup (k, c) takes the samples [k span, (k + 1) span) of row c: span / L whole buffers.  Readings that lie inside it are
// written; of a reading that reaches into a neighbour it leaves a partial (slot 0: the reading of its first buffer, slot 1: the
// reading of its last one) for levels_fold_kernel.
template <typename T>
__global__ void __launch_bounds__(256)
levels_in_kernel(const T *__restrict__ samples, int64_t n_samples, int64_t stride, int L, int64_t P, int64_t B,
                 double *__restrict__ out, int64_t M, LevelsPartial *__restrict__ part)
{
    constexpr int G = 16 / (int)sizeof(T);             // samples per 16-byte group
    constexpr int kSpan = kLevelsSpanBytes / (int)sizeof(T);
    constexpr int kReach = 64 * G;                     // samples of one wave in one pass
    __shared__ float sums[kSpan / 8];                  // one per min(L, kReach) samples
    const int c = blockIdx.y, tid = threadIdx.x;
    const T *row = samples + (int64_t)c * stride;
    const bool aligned = (reinterpret_cast<uintptr_t>(row) & 15u) == 0;
    const int64_t s0 = (int64_t)blockIdx.x * kSpan;

    u32x4 raw[kLevelsPasses];
#pragma unroll
    for (int j = 0; j < kLevelsPasses; j++) {
        const int64_t s = s0 + (int64_t)(j * 256 + tid) * G;
        if (aligned && s + G <= n_samples) raw[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(row + s));
        else if (s < n_samples) raw[j] = load_each(row, s, (int)min((int64_t)G, n_samples - s));
        else raw[j] = u32x4{0u, 0u, 0u, 0u};
    }
    const int lpb = L / G;                             // lanes a buffer (1: a lane holds a whole buffer of 8 int16)
    const int lead = min(lpb, 64), lead_shift = __ffs(lead) - 1;
#pragma unroll
    for (int j = 0; j < kLevelsPasses; j++) {
        const float p = lanes_sum<T>(raw[j], lpb);
        if ((tid & (lead - 1)) == 0) sums[(j * 256 + tid) >> lead_shift] = p;
    }
    __syncthreads();
    // buffers longer than a wave's reach: r consecutive wave sums each, the tree's upper levels in LDS
    const int r = lds_tree<kSpan, kReach>(sums, L, tid);
    const int bpb = kSpan / L;
    const int64_t b0 = (int64_t)blockIdx.x * bpb, bE = min(b0 + bpb, B);
    // Double(sum) / Double(length): the row's last buffer divides by its own length
    auto value = [&](int64_t b) {
        const int64_t len = b == B - 1 ? n_samples - b * L : (int64_t)L;
        return (double)sums[(int)(b - b0) * r] / (double)len;
    };
    const int64_t m0 = b0 / P, m1 = (bE - 1) / P;
    const int nr = (int)(m1 - m0 + 1);
    // `best`: the greatest value of [lo, hi) that is not NaN (-1: none; a mean square is never negative)
    auto emit = [&](int64_t m, int64_t lo, double best) {
        const bool has_first = lo == m * P;
        const double first = has_first ? value(lo) : 0.0;
        if (has_first && min((m + 1) * P, B) <= bE) out[(int64_t)c * M + m] = first != first ? first : best;
        else part[((int64_t)c * gridDim.x + blockIdx.x) * 2 + (m == m0 ? 0 : 1)] = LevelsPartial{best, first};
    };
    if (P < 16) {
        // short readings: a lane each
        for (int i = tid; i < nr; i += 256) {
            const int64_t m = m0 + i, lo = max(m * P, b0), hi = min((m + 1) * P, bE);
            const double best = best_of_lane(lo, hi, value);
            emit(m, lo, best);
        }
    } else {
        // long readings: a wave each (the greatest of values that are not NaN does not depend on the order)
        const int lane = tid & 63;
        for (int i = tid >> 6; i < nr; i += 4) {
            const int64_t m = m0 + i, lo = max(m * P, b0), hi = min((m + 1) * P, bE);
            const double best = best_of_wave(lo, hi, lane, value);
            if (lane == 0) emit(m, lo, best);
        }
    }
}

// Wave (k, c): if a reading begins in workgroup k of levels_in_kernel and ends behind it, this wave folds it -- its first value from
// workgroup k's partial, the greatest of the partials of workgroups k .. k1.
__global__ void __launch_bounds__(256)
levels_fold_kernel(const LevelsPartial *__restrict__ part, int nblocks, int bpb, int64_t B, int64_t P, double *__restrict__ out, int64_t M)
{
    const int c = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t k = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= nblocks) return;
    const int64_t b0 = k * bpb, bE = min(b0 + bpb, B);
    const int64_t m = (bE - 1) / P, f = m * P, e = min(f + P, B);
    if (f < b0 || e <= bE) return;                     // it began earlier, or lies inside the workgroup (written there)
    const int64_t k1 = (e - 1) / bpb;
    const LevelsPartial *row = part + (int64_t)c * nblocks * 2;
    const int slot = m == b0 / P ? 0 : 1;
    const double first = row[k * 2 + slot].first;
    double best = -1.0;
    for (int64_t j = k + lane; j <= k1; j += 64) {
        const double v = row[j * 2 + (j == k ? slot : 0)].best;
        if (v > best) best = v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(best, d);
        if (o > best) best = o;
    }
    if (lane == 0) out[(int64_t)c * M + m] = first != first ? first : best;
}

// Reading m of channel c: the evaluations [ce(min(m P L, S)), ce(min((m + 1) P L, S))), each cut at n_evals, where ce is
// syldet_count_evals (`need` = gap + window).  StatMax: the first value if it is NaN, else the first of the greatest values that are
// not NaN (a later equal value does not replace: -0 in front of +0 stays).  No evaluation: 0.  WAVE: a wave a reading, else a lane.
template <bool WAVE>
__global__ void __launch_bounds__(256)
levels_out_kernel(const float *__restrict__ outputs, int64_t n_evals, int n_out, int k, int64_t n_samples, int64_t PL, int64_t need,
                  int64_t hop, int T, float *__restrict__ levels, int64_t M)
{
    const int c = blockIdx.y, lane = WAVE ? (int)(threadIdx.x & 63) : 0;
    const int64_t m = WAVE ? (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6) : (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    const float result = levels_out_value<WAVE>(outputs + (int64_t)c * n_evals * n_out + k, n_evals, n_out, m, n_samples, PL, need, hop, T, lane);
    if (lane == 0) levels[(int64_t)c * M + m] = result;
}

int levels_span(bool s16) { return kLevelsSpanBytes / (s16 ? 2 : 4); }

// workgroups a row of levels_in_kernel (B buffers of L samples)
static int64_t levels_blocks(int64_t B, int L, bool s16) { return (B + levels_span(s16) / L - 1) / (levels_span(s16) / L); }

size_t levels_scratch_bytes(int64_t n_samples, int C, int L, bool s16)
{
    const int64_t B = (n_samples + L - 1) / L;
    return (size_t)std::max<int64_t>(1, levels_blocks(B, L, s16)) * (size_t)C * 2 * sizeof(LevelsPartial);
}

hipError_t launch_levels_in(const void *samples, bool s16, int C, int64_t n_samples, int64_t stride, int L, int64_t P, double *mean_square,
                            void *scratch, hipStream_t stream, bool *needs_fold)
{
    if (needs_fold) *needs_fold = false;
    if (n_samples <= 0 || C <= 0) return hipSuccess;
    if (L < 8 || L > 4096 || (L & (L - 1)) != 0 || P < 1 || (C > 1 && stride < n_samples) || C > 65535 ||
        (reinterpret_cast<uintptr_t>(samples) & (s16 ? 1u : 3u)) != 0)
        return hipErrorInvalidValue;
    const int64_t B = (n_samples + L - 1) / L;
    P = std::min(P, B);                                // (one reading either way; keeps m P inside 64 bits)
    const int64_t M = (B + P - 1) / P, blocks = levels_blocks(B, L, s16);
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    LevelsPartial *part = static_cast<LevelsPartial *>(scratch);
    if (s16)
        hipLaunchKernelGGL(levels_in_kernel<int16_t>, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, stream, (const int16_t *)samples,
                           n_samples, stride, L, P, B, mean_square, M, part);
    else
        hipLaunchKernelGGL(levels_in_kernel<float>, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, stream, (const float *)samples,
                           n_samples, stride, L, P, B, mean_square, M, part);
    // a reading crosses workgroups only where there are two of them, and not where every workgroup holds whole readings
    const int bpb = levels_span(s16) / L;
    if (needs_fold) *needs_fold = blocks >= 2 && !(P <= bpb && bpb % P == 0);
    return hipGetLastError();
}

hipError_t launch_levels_fold(const void *scratch, bool s16, int C, int64_t n_samples, int L, int64_t P, double *mean_square, hipStream_t stream)
{
    const int64_t B = (n_samples + L - 1) / L;
    P = std::min(P, B);
    const int64_t M = (B + P - 1) / P, blocks = levels_blocks(B, L, s16);
    hipLaunchKernelGGL(levels_fold_kernel, dim3((unsigned)((blocks + 3) / 4), (unsigned)C), dim3(256), 0, stream,
                       static_cast<const LevelsPartial *>(scratch), (int)blocks, levels_span(s16) / L, B, P, mean_square, M);
    return hipGetLastError();
}

hipError_t launch_levels_out(const float *outputs, int64_t n_evals, int n_out, int k, int C, int64_t n_samples, int L, int64_t P,
                             int64_t need, int64_t hop, int T, float *levels, hipStream_t stream)
{
    if (n_samples <= 0 || C <= 0) return hipSuccess;
    if (L < 8 || L > 4096 || (L & (L - 1)) != 0 || P < 1 || n_evals < 0 || n_out < 1 || k < 0 || k >= n_out || hop < 1 || T < 1 || C > 65535)
        return hipErrorInvalidValue;
    const int64_t B = (n_samples + L - 1) / L;
    P = std::min(P, B);
    const int64_t M = (B + P - 1) / P, PL = P * L;
    // a wave a reading where readings hold more than a few evaluations
    const bool wave = n_evals / M > 8;
    const int64_t blocks = wave ? (M + 3) / 4 : (M + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (wave)
        hipLaunchKernelGGL(levels_out_kernel<true>, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, stream, outputs, n_evals, n_out, k,
                           n_samples, PL, need, hop, T, levels, M);
    else
        hipLaunchKernelGGL(levels_out_kernel<false>, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, stream, outputs, n_evals, n_out, k,
                           n_samples, PL, need, hop, T, levels, M);
    return hipGetLastError();
}

}  // namespace sd
