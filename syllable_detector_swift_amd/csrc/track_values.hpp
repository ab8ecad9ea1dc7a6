// track_values.hpp -- the value arithmetic of the two per-sample tracks, shared by the kernels that write one recording a row
// (kernels_trace.hip, kernels_trigger.hip) and the kernels that write the recordings of a packed bank
// (kernels_recordings_tracks.hip): one statement of each value, so the two paths cannot drift apart.
//   trace_word           one evaluation of the Simulator's output track (ViewControllerSimulator.swift:322-328)
//   trigger_scan_row     flags of one recording -> its last_seen table (Processor.swift:128-148)
//   trigger_high         one sample of the trigger track's closed form (AudioInterface.swift:13-40, :442-445)
//   trigger_onsets_row   the rising edges of one recording, in order
// Every file that includes it is compiled with -ffp-contract=off and without fast-math (see the Makefile): the trace's `/` is the
// correctly rounded fp32 division, and its product with 32767 rounds on its own.
//
// gfx950 only.  wave = 64, workgroups of 256 lanes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sd {

// n / d for n d < 2^32 as one multiplication (magic = ceil(2^32 / d)); magic == 0: d == 1 or a pair too large for it
__device__ __forceinline__ unsigned div_magic(unsigned n, unsigned d, unsigned magic)
{
    return magic ? __umulhi(n, magic) : n / d;
}

// ceil(2^32 / d) where n / d == umulhi(n, magic) for every n < bound (n d < 2^32), else 0: the kernels divide then
inline unsigned magic_for(uint64_t bound, unsigned d)
{
    if (d <= 1 || bound * d >= (1ull << 32)) return 0u;
    return (unsigned)(((1ull << 32) + d - 1) / d);
}

// The 32-bit word LDS holds for evaluation e of a row: the value's bits (fp32 trace) or its 16-bit sample (int16 trace).
// Evaluations past n_evals are 0 (samples behind the last hold).
template <bool S16>
__device__ __forceinline__ unsigned trace_word(const float *__restrict__ row, int64_t e, int64_t n_evals, int n_out, float thr)
{
    if (e >= n_evals) return 0u;
    float v = row[e * n_out] / thr;
    if (v > 1.0f) v = 1.0f;                    // :323-325
    if (v < 0.0f) v = 0.0f;                    // :326-328
    if (!S16) return __float_as_uint(v);
    // this project's 16-bit form: rint(v * 32767), ties to even, NaN -> 0 (v is in [0, 1] or NaN here)
    const float x = (v != v) ? 0.0f : v;
    return (unsigned)(int)rintf(x * 32767.0f);
}

constexpr int kScanItems = 8;             // buffers a lane scans in a row ...
constexpr int kScanChunk = 256 * kScanItems;   // ... and a workgroup per step

// inclusive scan of one int a lane over the 256 lanes of a workgroup (Hillis-Steele in LDS); MAX: maximum, else sum
template <bool MAX>
__device__ __forceinline__ int block_scan(int v, int *buf, int tid)
{
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < 256; d <<= 1) {
        const int o = tid >= d ? buf[tid - d] : (MAX ? -1 : 0);
        __syncthreads();
        v = MAX ? max(v, o) : v + o;
        buf[tid] = v;
        __syncthreads();
    }
    return v;
}

// ceil(a / d) for d >= 1, 0 for a <= 0
__device__ __forceinline__ int64_t ceil_div_pos(int64_t a, int64_t d) { return a <= 0 ? 0 : (a + d - 1) / d; }

// One workgroup, one recording: fl [n_evals] its flags, out [Bp] its last_seen table; seen [kScanChunk] and buf [256] in LDS.  A chunk
// of buffers [b0, b0 + kScanChunk): the evaluations that become available in them are read once, in order (a byte a lane), and
// mark their buffer in LDS; then a max-scan along the chunk with the carry of the chunks before.  No flag outside [0, n_evals) is read.
__device__ __forceinline__ void trigger_scan_row(const uint8_t *__restrict__ fl, int64_t n_evals, int64_t D, int64_t hop, int lgL,
                                                 int *__restrict__ out, int Bp, int *seen, int *buf, int tid)
{
    int carry = -1;
    for (int b0 = 0; b0 < Bp; b0 += kScanChunk) {
        const int nb = min(kScanChunk, Bp - b0);
        for (int i = tid; i < kScanChunk; i += 256) seen[i] = -1;
        __syncthreads();
        // evaluations e with b0 <= b(e) < b0 + nb:  D + e hop - 1 >= b0 L  <=>  e >= ceil((b0 L + 1 - D) / hop)
        const int64_t e_lo = min(ceil_div_pos(((int64_t)b0 << lgL) + 1 - D, hop), n_evals);
        const int64_t e_hi = min(ceil_div_pos(((int64_t)(b0 + nb) << lgL) + 1 - D, hop), n_evals);
        for (int64_t e = e_lo + tid; e < e_hi; e += 256)
            if (fl[e] != 0) {
                const int64_t b = max(D + e * hop - 1, (int64_t)0) >> lgL;
                const int64_t i = b - b0;
                if (i >= 0 && i < nb) seen[i] = (int)b;        // (lanes that meet in a buffer write the same value)
            }
        __syncthreads();
        int run = -1;
#pragma unroll
        for (int j = 0; j < kScanItems; j++) {
            run = max(run, seen[tid * kScanItems + j]);
            seen[tid * kScanItems + j] = run;
        }
        const int incl = block_scan<true>(run, buf, tid);
        (void)incl;
        const int before = max(carry, tid > 0 ? buf[tid - 1] : -1);
        const int total = buf[255];
#pragma unroll
        for (int j = 0; j < kScanItems; j++) seen[tid * kScanItems + j] = max(seen[tid * kScanItems + j], before);
        __syncthreads();
        for (int i = tid; i < nb; i += 256) out[b0 + i] = seen[i];
        carry = max(carry, total);
        __syncthreads();
    }
}

// one sample of the closed form: the table through `at` (an index into the recording's last_seen table, already clamped)
template <class At>
__device__ __forceinline__ bool trigger_high(int64_t s, int64_t Lat, int lgL, int64_t N, At at)
{
    const int64_t u = s - Lat;
    if (u < ((int64_t)1 << lgL)) return false;
    const int b = at((u >> lgL) - 1);
    return b >= 0 && s < (((int64_t)b + 1) << lgL) + Lat + N;
}

// One workgroup, one recording: buffer b is an onset iff it is seen (last_seen[b] == b), its pulse starts inside the recording and
// no seen buffer lies in [b - N / L, b).  A lane tests kScanItems buffers in a row; a prefix sum over the workgroup and the
// carry of the chunks before put the onsets in order.  idx [capacity]: the first min(count, capacity); returns the count.
__device__ __forceinline__ int64_t trigger_onsets_row(const int *__restrict__ row, int Bp, int lgL, int64_t N, int64_t Lat, int64_t n_samples,
                                                      int64_t *__restrict__ idx, int64_t capacity, int *buf, int tid)
{
    const int64_t K = N >> lgL;
    int64_t carry = 0;
    for (int b0 = 0; b0 < Bp; b0 += kScanChunk) {
        const int first = b0 + tid * kScanItems;
        unsigned mask = 0u;
        int prev = (first > 0 && first <= Bp) ? row[first - 1] : -1;
#pragma unroll
        for (int j = 0; j < kScanItems; j++) {
            const int b = first + j;
            if (b < Bp) {
                const int cur = row[b];
                const int64_t t = (((int64_t)b + 1) << lgL) + Lat;
                if (cur == b && t < n_samples && (prev < 0 || (int64_t)prev < (int64_t)b - K)) mask |= 1u << j;
                prev = cur;
            }
        }
        const int mine = __popc(mask);
        const int incl = block_scan<false>(mine, buf, tid);
        const int total = buf[255];
        int64_t at = carry + (incl - mine);
#pragma unroll
        for (int j = 0; j < kScanItems; j++)
            if (mask & (1u << j)) {
                if (at < capacity) idx[at] = (((int64_t)(first + j) + 1) << lgL) + Lat;
                at++;
            }
        carry += total;
        __syncthreads();
    }
    return carry;
}

}  // namespace sd
