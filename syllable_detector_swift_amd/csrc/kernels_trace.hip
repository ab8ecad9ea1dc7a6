// kernels_trace.hip -- the Simulator's output track (SyllableDetector/ViewControllerSimulator.swift:251-344): the detector's
// output k as a fraction of its threshold, held from one evaluation to the next, one value per audio sample.
//   trace_kernel                     planar rows [C][stride], fp32 (the reference's floats) or int16 (rint(v * 32767))
//   trace_interleaved_s16_kernel     frame-major [n_samples][C] int16, the layout a 16-bit WAV stores
// With D = first_index (the Simulator's nextCount, :251-254) and hop = windowLength - windowOverlap (:331):
//   v[e]     = clamp01(out[e][k] / Float(thr[k]))          :322-328 (two comparisons: NaN stays NaN)
//   trace[s] = 0 for s < D,  v[(s - D) / hop] for D <= s < D + n_evals hop,  0 beyond
// A write-bound expansion: 4 bytes read per evaluation, `hop` samples written.  A workgroup computes the evaluations its span of
// samples touches once, into LDS, and expands from there with 16-byte stores.
//
// gfx950 only.  wave = 64.

#include <algorithm>

#include "kernels.hpp"
#include "track_values.hpp"   // div_magic, magic_for, trace_word

// the division, the product with 32767 and the rounding each round on their own: this file is compiled with
// -ffp-contract=off (see the Makefile) and without any fast-math flag -- `/` is the correctly rounded fp32 division

namespace sd {

namespace {

constexpr int kTraceSpanBytes = 16384;    // bytes of one channel's row per workgroup (planar): four passes of 256 lanes x 16 bytes, the
                                          // fastest of 8 .. 256 KiB on 64 x 2^24 (MEASUREMENTS.md, "The Simulator's output track")
constexpr int kTraceEvals = 4096;         // evaluations a workgroup's samples may touch (a hop of 1 halves the int16 span: trace_span)
constexpr int kTraceTileCh = 64;          // interleaved: channels per tile ...
constexpr int kTraceTileEvals = 128;      // ... and evaluations per channel a tile may touch (its frames: trace_tile_frames)

// Planar rows.  Workgroup (b, c) writes the samples [head + b span, head + (b + 1) span) of row c, where `head` (< 16 bytes) is
// what lies in front of the row's first 16-byte line; workgroup 0 also writes the head.  Every lane stores one aligned group
// of 16 bytes per pass; the head and the row's last partial group go sample by sample.  `span` (trace_span) keeps the
// evaluations of a workgroup within kTraceEvals.
template <typename T>
__global__ void __launch_bounds__(256)
trace_kernel(const float *__restrict__ outputs, int64_t n_evals, int n_out, int k, const float *__restrict__ thr,
             T *__restrict__ trace, int64_t n_samples, int64_t stride, int64_t D, unsigned hop, unsigned hop_magic, int span)
{
    constexpr bool S16 = sizeof(T) == 2;
    constexpr int G = 16 / (int)sizeof(T);             // samples per 16-byte group
    __shared__ unsigned ev[kTraceEvals + 16];
    const int c = blockIdx.y, tid = threadIdx.x;
    T *dst = trace + (int64_t)c * stride;
    const int64_t head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / (int64_t)sizeof(T);
    const int64_t g0 = head + (int64_t)blockIdx.x * span;                // first aligned sample of this workgroup
    const int64_t sA = blockIdx.x == 0 ? 0 : g0;
    const int64_t sB = min(g0 + (int64_t)span, n_samples);
    if (sA >= sB) return;
    // the evaluations [eA, eA + nE) the span touches: the one full division of the workgroup (32-bit where the row allows)
    const int64_t first = max(sA, D);
    const uint64_t ahead = (uint64_t)(first - D);
    const int64_t eA = (ahead >> 32) == 0 ? (int64_t)((unsigned)ahead / hop) : (int64_t)(ahead / hop);
    const int64_t base = D + eA * (int64_t)hop;                          // first sample of evaluation eA: first - hop < base <= first
    const int nE = sB > D ? (int)div_magic((unsigned)(sB - 1 - base), hop, hop_magic) + 1 : 0;
    const float *row = outputs + (int64_t)c * n_evals * n_out + k;
    const float t = thr[c];
    for (int i = tid; i < nE; i += 256) ev[i] = trace_word<S16>(row, eA + i, n_evals, n_out, t);
    __syncthreads();
    auto store_each = [&](int64_t s, int n, const unsigned *w) {
#pragma unroll
        for (int j = 0; j < G; j++)
            if (j < n) {
                if (S16) reinterpret_cast<uint16_t *>(dst)[s + j] = (uint16_t)w[j];
                else reinterpret_cast<unsigned *>(dst)[s + j] = w[j];
            }
    };
    auto store_group = [&](int64_t s, const unsigned *w) {
        uint4 v;
        if (S16) v = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
        else v = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4 *>(dst + s) = v;
    };
    // the value of sample s >= D: ev[(s - base) / hop]; a group walks on from its first sample's quotient and remainder
    unsigned w[G];
    auto expand = [&](int64_t s, int n) {
        const int64_t rel = s - base;                                    // negative only in front of D (base is D there)
        const int lead = rel < 0 ? (int)min((int64_t)n, -rel) : 0;
        const unsigned r = rel < 0 ? 0u : (unsigned)rel;
        unsigned e = div_magic(r, hop, hop_magic), rem = r - e * hop;
#pragma unroll
        for (int j = 0; j < G; j++) {
            const bool live = j >= lead && j < n;
            w[j] = live ? ev[e] : 0u;
            if (live && ++rem == hop) { rem = 0; e++; }
        }
    };
    // the row's head and its last partial group, sample by sample: one lane each
    const int64_t whole = g0 + ((sB - g0) & ~(int64_t)(G - 1));         // end of the workgroup's whole groups (sB <= g0: none)
    if (blockIdx.x == 0 && tid == 0 && head > 0) {
        const int n = (int)min(head, n_samples);
        expand(0, n);
        store_each(0, n, w);
    }
    if (tid == 64 && sB > whole && whole >= g0) {
        expand(whole, (int)(sB - whole));
        store_each(whole, (int)(sB - whole), w);
    }
    if (sA >= D && hop >= (unsigned)G && hop_magic != 0u) {
        // every workgroup behind D where a hold is at least a group long (workgroup-uniform): a group lies in two evaluations at most
        for (int64_t s = g0 + (int64_t)tid * G; s < whole; s += 256 * G) {
            const unsigned r = (unsigned)(s - base);
            const unsigned e = __umulhi(r, hop_magic);
            const unsigned left = hop - (r - e * hop);                   // samples of the group's first evaluation from s on
            // (b is read even where the whole group lies in evaluation e: left >= G never selects it.  Behind the span's last
            // evaluation e + 1 == nE, a word no lane wrote, inside the array by the 16 words of slack behind kTraceEvals)
            const unsigned a = ev[e], b = ev[e + 1];
#pragma unroll
            for (int j = 0; j < G; j++) w[j] = (unsigned)j < left ? a : b;
            store_group(s, w);
        }
        return;
    }
    for (int64_t s = g0 + (int64_t)tid * G; s < whole; s += 256 * G) {
        expand(s, G);
        store_group(s, w);
    }
}

// Frame-major int16.  A workgroup takes a tile of `tile_frames` frames x up to 64 channels: the evaluations of every channel of
// the tile go into LDS channel by channel (deinterleave_s16_kernel run backwards: LDS is filled along the channels' rows and read
// along the frames), then consecutive lanes store consecutive 16-byte groups of the frame-major buffer.  Up to 64 channels a
// tile holds whole frames, one contiguous run of the buffer; wider banks are written as row segments of 64 channels.
__global__ void __launch_bounds__(256)
trace_interleaved_s16_kernel(const float *__restrict__ outputs, int64_t n_evals, int n_out, int k, const float *__restrict__ thr,
                             int16_t *__restrict__ frames, int64_t n_frames, int C, int64_t D, unsigned hop, unsigned hop_magic,
                             int tile_frames, unsigned c_magic)
{
    constexpr int P = kTraceTileEvals + 1;             // odd pitch: lanes on consecutive channels read different banks
    __shared__ unsigned ev[kTraceTileCh * P];
    const int tid = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * tile_frames;
    const int c0 = blockIdx.y * kTraceTileCh;
    const int nc = min(kTraceTileCh, C - c0);
    const int nf = (int)min((int64_t)tile_frames, n_frames - f0);
    const int64_t fB = f0 + nf;
    const int64_t first = max(f0, D);
    const int64_t eA = (first - D) / (int64_t)hop;                        // (the one 64-bit division of the workgroup)
    const int64_t base = D + eA * (int64_t)hop;
    const int nE = fB > D ? (int)div_magic((unsigned)(fB - 1 - base), hop, hop_magic) + 1 : 0;   // <= kTraceTileEvals (trace_tile_frames)
    for (int i = tid; i < nc * nE; i += 256) {
        const int ch = i / nE, el = i - ch * nE;
        ev[ch * P + el] = trace_word<true>(outputs + (int64_t)(c0 + ch) * n_evals * n_out + k, eA + el, n_evals, n_out, thr[c0 + ch]);
    }
    __syncthreads();
    // rows of the tile in the frame-major buffer: one of nf * C samples (whole frames), or nf of nc samples each
    const bool flat = nc == C;
    const unsigned row_len = flat ? (unsigned)nf * (unsigned)C : (unsigned)nc;
    const unsigned gpr = (row_len + 7u) >> 3, rows = flat ? 1u : (unsigned)nf;
    const unsigned gpr_magic = (!flat && gpr > 1u) ? 0xffffffffu / gpr + 1u : 0u;
    for (unsigned g = tid; g < rows * gpr; g += 256) {
        const unsigned row = flat ? 0u : div_magic(g, gpr, gpr_magic);
        const unsigned i0 = (g - row * gpr) << 3;
        const int n = (int)min(8u, row_len - i0);
        unsigned f = flat ? div_magic(i0, (unsigned)C, c_magic) : row;    // the group's first frame and channel (of the tile)
        unsigned ch = flat ? i0 - f * (unsigned)C : i0;
        int16_t *p = frames + (f0 + (flat ? 0 : (int64_t)row)) * C + c0 + i0;
        // the first frame's evaluation; frames in front of D are 0
        const int64_t rel = f0 + (int64_t)f - base;
        int lead = rel < 0 ? (int)min((int64_t)0x7fffffff, -rel) : 0;   // frames still to go before D
        unsigned e = 0, rem = 0;
        if (rel >= 0) {
            e = div_magic((unsigned)rel, hop, hop_magic);
            rem = (unsigned)rel - e * hop;
        }
        unsigned w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            w[j] = (j < n && lead == 0) ? ev[ch * P + e] : 0u;
            if (++ch == (unsigned)nc) {                                   // next frame (only whole-frame tiles get here inside a group)
                ch = 0;
                if (lead > 0) lead--;
                else if (++rem == hop) { rem = 0; e++; }
            }
        }
        if (n == 8 && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
        } else {
#pragma unroll
            for (int j = 0; j < 8; j++)
                if (j < n) reinterpret_cast<uint16_t *>(p)[j] = (uint16_t)w[j];
        }
    }
}

// samples per workgroup of the planar kernel: a span of n samples (and a head of up to 7) touches at most (n + 5) / hop + 2
// evaluations, kept within kTraceEvals + 16
int trace_span(int64_t hop, size_t sample_bytes)
{
    return (int)std::min<int64_t>(kTraceSpanBytes / (int64_t)sample_bytes, (int64_t)kTraceEvals * std::min<int64_t>(hop, 4));
}

// frames per tile of the interleaved kernel: a multiple of 8 (whole 16-byte groups for any channel count), at most 256, and
// few enough that a channel's evaluations fit the tile's LDS (a tile of n frames touches at most (n - 1) / hop + 2 evaluations)
int trace_tile_frames(int64_t hop)
{
    const int64_t most = (int64_t)(kTraceTileEvals - 2) * hop + 1;
    return (int)std::max<int64_t>(8, std::min<int64_t>(256, most) / 8 * 8);
}

}  // namespace

template <typename T>
static hipError_t launch_trace_t(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C, T *trace,
                                 int64_t n_samples, int64_t stride, int64_t first_index, int64_t hop, hipStream_t stream)
{
    if (n_samples <= 0 || C <= 0) return hipSuccess;
    if (hop < 1 || hop > 0x7fffffffLL - 2 * kTraceSpanBytes || first_index < 0 || n_evals < 0 || n_out < 1 || k < 0 || k >= n_out ||
        (C > 1 && stride < n_samples) || C > 65535 || (reinterpret_cast<uintptr_t>(trace) & (sizeof(T) - 1)) != 0)
        return hipErrorInvalidValue;
    const int span = trace_span(hop, sizeof(T));
    // (one more workgroup than n / span where a row's head shifts the spans)
    const int64_t blocks = (n_samples + span - 1) / span + 1;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned magic = magic_for((uint64_t)span + 16 + (uint64_t)hop, (unsigned)hop);
    hipLaunchKernelGGL(trace_kernel<T>, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, stream, outputs, n_evals, n_out, k, thr, trace,
                       n_samples, stride, first_index, (unsigned)hop, magic, span);
    return hipGetLastError();
}

hipError_t launch_trace(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C, float *trace,
                        int64_t n_samples, int64_t stride, int64_t first_index, int64_t hop, hipStream_t stream)
{
    return launch_trace_t<float>(outputs, n_evals, n_out, k, thr, C, trace, n_samples, stride, first_index, hop, stream);
}

hipError_t launch_trace_s16(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C, int16_t *trace,
                            int64_t n_samples, int64_t stride, int64_t first_index, int64_t hop, hipStream_t stream)
{
    return launch_trace_t<int16_t>(outputs, n_evals, n_out, k, thr, C, trace, n_samples, stride, first_index, hop, stream);
}

hipError_t launch_trace_interleaved_s16(const float *outputs, int64_t n_evals, int n_out, int k, const float *thr, int C,
                                        int16_t *frames, int64_t n_frames, int64_t first_index, int64_t hop, hipStream_t stream)
{
    if (n_frames <= 0 || C <= 0) return hipSuccess;
    // one channel: the frame-major buffer is the planar row
    if (C == 1) return launch_trace_s16(outputs, n_evals, n_out, k, thr, 1, frames, n_frames, n_frames, first_index, hop, stream);
    if (hop < 1 || hop > 0x7fffffffLL - 512 || first_index < 0 || n_evals < 0 || n_out < 1 || k < 0 || k >= n_out || C > 65535 ||
        (reinterpret_cast<uintptr_t>(frames) & 1) != 0)
        return hipErrorInvalidValue;
    const int tf = trace_tile_frames(hop);
    const int64_t tiles = (n_frames + tf - 1) / tf;
    const int ctiles = (C + kTraceTileCh - 1) / kTraceTileCh;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const unsigned magic = magic_for((uint64_t)tf + (uint64_t)hop, (unsigned)hop);
    const unsigned c_magic = magic_for((uint64_t)tf * kTraceTileCh + 8, (unsigned)C);
    hipLaunchKernelGGL(trace_interleaved_s16_kernel, dim3((unsigned)tiles, (unsigned)ctiles), dim3(256), 0, stream, outputs, n_evals, n_out,
                       k, thr, frames, n_frames, C, first_index, (unsigned)hop, magic, tf, c_magic);
    return hipGetLastError();
}

}  // namespace sd
