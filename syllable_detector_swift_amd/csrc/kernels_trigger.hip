// kernels_trigger.hip -- the TTL trigger track: the pulses the reference's rig emits for its detections (Processor.swift:128-148
// sets `seen` for a callback buffer, ProcessorAudio.prepareOutputFor :217-221 arms a pulse, AudioInterface.swift:442-445 sets
// outputHighFor = Int(duration * rate), renderOutput :13-40 writes 1.0 for that many samples from the next render buffer on).
//   trigger_scan_kernel                 last_seen [C][B'] int32: the greatest seen buffer <= b, or -1
//   trigger_kernel<T>                   planar rows [C][stride], fp32 (1.0f / 0.0f) or int16 (32767 / 0)
//   trigger_interleaved_s16_kernel<MUX> frame-major int16 [n_samples][C]; MUX: [n_samples][2 C], audio and trigger alternating
//   trigger_onsets_kernel               the rising edges, in order, as sample numbers (the convention of detections_kernel)
// With D = first_index, hop, callback buffers of L samples (a power of two), pulse width N and output latency Lat (include/syldet.h):
//   b(e)      = (D + e hop - 1) / L                      the buffer whose callback makes evaluation e available
//   seen(b)   = some e < n_evals with b(e) = b has flags[e] != 0
//   t_b       = (b + 1) L + Lat                          the first sample of the render buffer behind a seen buffer's callback
//   track[s]  = 1 iff some seen b has t_b <= s < t_b + N
// The closed form the expansion kernels evaluate.  t_b <= s  <=>  (b + 1) L <= s - Lat  <=>  b <= q, q = (s - Lat) / L - 1 (and no
// b at all while s - Lat < L).  Of the seen buffers <= q the greatest, b* = last_seen[q], ends last (t_b + N grows with b), so
//   track[s] = 1  <=>  s - Lat >= L  and  b* >= 0  and  s < (b* + 1) L + Lat + N
// (q <= (n_samples - 1) / L - 1 < B' = ceil((n_samples + L - 1) / L): the table covers every q a sample asks for; the kernels
// clamp the index to B' - 1 all the same).  outputHighFor is set, not added to (:444): a later arm inside a pulse moves its end
// to t_b + N of its own, which is the union above.  The table is what makes N and Lat free: no kernel behind the scan looks
// back over flags, so a pulse longer than a workgroup's span, or one that starts in another workgroup's span, is one table read.
// An onset is a seen buffer b with no seen buffer in [b - N / L, b) (pulses that abut are one pulse): last_seen[b - 1] < b - N / L.
//
// The scan is one workgroup a channel that walks the buffers in chunks of kScanChunk and carries the running maximum: no
// workgroup waits for another one, so nothing can spin.  A decoupled look-back scan would spread a channel over the device; it
// was not built (MEASUREMENTS.md, "The trigger track", says what the one-workgroup walk costs).
//
// gfx950 only.  wave = 64.  Every value is written with ordinary vector stores.

#include <algorithm>

#include "kernels.hpp"
#include "track_values.hpp"   // the scan, trigger_high and the onsets of one recording

namespace sd {

namespace {

constexpr int kTrigSpanBytes = 16384;     // bytes of one channel's row per workgroup (planar): the trace's span (kTraceSpanBytes)
constexpr int kTrigSlice = kTrigSpanBytes / 2 / 8 + 8;   // table entries a span may touch: span / L + 2 at L = 8, int16, and slack
constexpr int kTrigTileCh = 64;           // interleaved: channels per tile ...
constexpr int kTrigTileFrames = 256;      // ... and frames (a multiple of 8: whole 16-byte groups for any channel count)
constexpr int kTrigTileSlice = kTrigTileFrames / 8 + 2;   // table entries of one channel a tile may touch (L = 8)

// One workgroup a channel.  A chunk of buffers [b0, b0 + kScanChunk): the evaluations that become available in them are read
// once, in order (a byte a lane), and mark their buffer in LDS; then a max-scan along the chunk with the carry of the chunks before.
__global__ void __launch_bounds__(256)
trigger_scan_kernel(const uint8_t *__restrict__ flags, int64_t n_evals, int64_t D, int64_t hop, int lgL, int *__restrict__ last_seen,
                    int Bp)
{
    __shared__ int seen[kScanChunk];
    __shared__ int buf[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const uint8_t *fl = flags + (int64_t)c * n_evals;
    int *out = last_seen + (int64_t)c * Bp;
    trigger_scan_row(fl, n_evals, D, hop, lgL, out, Bp, seen, buf, tid);
}

// Planar rows; the structure of trace_kernel.  Workgroup (b, c) writes the samples [head + b span, head + (b + 1) span) of row c,
// `head` (< 16 bytes) being what lies in front of the row's first 16-byte line; workgroup 0 also writes the head.  The slice of
// last_seen its samples ask for goes into LDS first.  A group of 16 bytes holds at most 8 <= L samples, so it lies in two table
// entries at most.
template <typename T>
__global__ void __launch_bounds__(256)
trigger_kernel(const int *__restrict__ last_seen, int Bp, T *__restrict__ track, int64_t n_samples, int64_t stride, int lgL, int64_t N,
               int64_t Lat, int span)
{
    constexpr bool S16 = sizeof(T) == 2;
    constexpr int G = 16 / (int)sizeof(T);
    constexpr unsigned kHigh = S16 ? 32767u : 0x3f800000u;      // 32767, or the bits of 1.0f
    __shared__ int ls[kTrigSlice];
    const int c = blockIdx.y, tid = threadIdx.x;
    T *dst = track + (int64_t)c * stride;
    const int64_t head = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u) / (int64_t)sizeof(T);
    const int64_t g0 = head + (int64_t)blockIdx.x * span;
    const int64_t sA = blockIdx.x == 0 ? 0 : g0;
    const int64_t sB = min(g0 + (int64_t)span, n_samples);
    if (sA >= sB) return;
    const int64_t L = (int64_t)1 << lgL;
    // table entries [qA, qA + nQ) of this span, and one more for the second half of a group (clamped to the row)
    const int64_t qA = sA - Lat >= L ? ((sA - Lat) >> lgL) - 1 : 0;
    const int64_t qB = sB - 1 - Lat >= L ? ((sB - 1 - Lat) >> lgL) - 1 : -1;
    const int nQ = qB >= qA ? (int)min(qB - qA + 2, (int64_t)kTrigSlice) : 0;
    const int *row = last_seen + (int64_t)c * Bp;
    for (int i = tid; i < nQ; i += 256) ls[i] = row[min(qA + i, (int64_t)Bp - 1)];
    __syncthreads();
    auto at = [&](int64_t q) { return ls[min(max(q - qA, (int64_t)0), (int64_t)(kTrigSlice - 1))]; };
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
    unsigned w[G];
    auto expand = [&](int64_t s, int n) {                       // sample by sample
#pragma unroll
        for (int j = 0; j < G; j++) w[j] = (j < n && nQ > 0 && trigger_high(s + j, Lat, lgL, N, at)) ? kHigh : 0u;
    };
    const int64_t whole = g0 + ((sB - g0) & ~(int64_t)(G - 1));
    if (blockIdx.x == 0 && tid == 0 && head > 0) {
        const int n = (int)min(head, n_samples);
        expand(0, n);
        store_each(0, n, w);
    }
    if (tid == 64 && sB > whole && whole >= g0) {
        expand(whole, (int)(sB - whole));
        store_each(whole, (int)(sB - whole), w);
    }
    for (int64_t s = g0 + (int64_t)tid * G; s < whole; s += 256 * G) {
        const int64_t u = s - Lat;
        if (nQ > 0 && u >= L) {
            // the group's first entry q0 holds its first `left` samples, q0 + 1 the rest; each entry's pulse ends at (b + 1) L + Lat + N
            const int64_t q0 = (u >> lgL) - 1;
            const int left = (int)(L - (u & (L - 1)));
            const int a = at(q0), b = at(q0 + 1);
            const int64_t ea = a >= 0 ? (((int64_t)a + 1) << lgL) + Lat + N - s : 0;   // samples of the group below a's end
            const int64_t eb = b >= 0 ? (((int64_t)b + 1) << lgL) + Lat + N - s : 0;
            const int ra = (int)min(max(ea, (int64_t)0), (int64_t)G), rb = (int)min(max(eb, (int64_t)0), (int64_t)G);
#pragma unroll
            for (int j = 0; j < G; j++) w[j] = (j < left ? j < ra : j < rb) ? kHigh : 0u;
        } else {
            expand(s, G);
        }
        store_group(s, w);
    }
}

// Frame-major int16; the structure of trace_interleaved_s16_kernel.  A workgroup takes a tile of up to 256 frames x up to 64
// channels: every channel's slice of last_seen goes into LDS channel by channel (and, MUX, the channel's audio of the tile's frames,
// read along its planar row), then consecutive lanes store consecutive 16-byte groups of the frame-major buffer.  A frame has
// W = C lanes (MUX: 2 C, channel ch at lane 2 ch its audio and at 2 ch + 1 its trigger).  Up to 64 channels a tile holds whole
// frames, one contiguous run of the buffer, and a group whose address is a multiple of 16 bytes is one 16-byte store (every group
// where the buffer's base and the tile's first frame are aligned: 256 W samples a tile).  Wider banks are written as row segments
// of the tile's lanes: a segment starts at (f W + 64 k V) samples, which is a multiple of 8 only for some W, and its groups are
// then stored sample by sample -- correct at any alignment, but not the 16-byte path (the segments' heads are not peeled).
template <bool MUX>
__global__ void __launch_bounds__(256)
trigger_interleaved_s16_kernel(const int *__restrict__ last_seen, int Bp, const int16_t *__restrict__ samples, int64_t sample_stride,
                               int16_t *__restrict__ frames, int64_t n_frames, int C, int lgL, int64_t N, int64_t Lat)
{
    constexpr int P = kTrigTileSlice + 1;              // 35, odd: lanes on consecutive channels read different banks
    constexpr int PA = kTrigTileFrames + 2;            // audio pitch in samples: 129 words, odd
    constexpr int V = MUX ? 2 : 1;                     // lanes of a frame a channel
    __shared__ int ls[kTrigTileCh * P];
    __shared__ int16_t au[MUX ? kTrigTileCh * PA : 2];
    const int tid = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * kTrigTileFrames;
    const int c0 = blockIdx.y * kTrigTileCh;
    const int nc = min(kTrigTileCh, C - c0);
    const int nf = (int)min((int64_t)kTrigTileFrames, n_frames - f0);
    if (nf <= 0 || nc <= 0) return;
    const int64_t fB = f0 + nf, L = (int64_t)1 << lgL;
    const int64_t qA = f0 - Lat >= L ? ((f0 - Lat) >> lgL) - 1 : 0;
    const int64_t qB = fB - 1 - Lat >= L ? ((fB - 1 - Lat) >> lgL) - 1 : -1;
    const int nQ = qB >= qA ? (int)min(qB - qA + 1, (int64_t)kTrigTileSlice) : 0;
    for (int i = tid; i < nc * nQ; i += 256) {
        const int ch = i / nQ, k = i - ch * nQ;
        ls[ch * P + k] = last_seen[(int64_t)(c0 + ch) * Bp + min(qA + k, (int64_t)Bp - 1)];
    }
    if (MUX)
        for (int i = tid; i < nc * nf; i += 256) {
            const int ch = i / nf, k = i - ch * nf;
            au[ch * PA + k] = samples[(int64_t)(c0 + ch) * sample_stride + f0 + k];
        }
    __syncthreads();
    const unsigned W = (unsigned)C * V, nw = (unsigned)nc * V;
    const bool flat = nc == C;
    const unsigned row_len = flat ? (unsigned)nf * W : nw;
    const unsigned gpr = (row_len + 7u) >> 3, rows = flat ? 1u : (unsigned)nf;
    for (unsigned g = tid; g < rows * gpr; g += 256) {
        const unsigned row = flat ? 0u : g / gpr;
        const unsigned i0 = (g - row * gpr) << 3;
        const int n = (int)min(8u, row_len - i0);
        unsigned f = flat ? i0 / W : row;                                 // the group's first frame (of the tile) and lane (of the tile)
        unsigned lane = flat ? i0 - f * W : i0;
        int16_t *p = frames + (f0 + (flat ? 0 : (int64_t)row)) * W + (int64_t)c0 * V + i0;
        unsigned w[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            unsigned v = 0u;
            if (j < n) {
                const int ch = (int)(lane / V);
                if (MUX && (lane & 1u) == 0u) {
                    v = (uint16_t)au[ch * PA + (int)f];
                } else {
                    auto at = [&](int64_t q) { return ls[ch * P + (int)min(max(q - qA, (int64_t)0), (int64_t)(kTrigTileSlice - 1))]; };
                    v = (nQ > 0 && trigger_high(f0 + f, Lat, lgL, N, at)) ? 32767u : 0u;
                }
            }
            w[j] = v;
            if (++lane == nw) { lane = 0; f++; }                          // (only whole-frame tiles get here inside a group)
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

// One workgroup a channel: buffer b is an onset iff it is seen (last_seen[b] == b), its pulse starts inside the recording and
// no seen buffer lies in [b - N / L, b).  A lane tests kScanItems buffers in a row; a prefix sum over the workgroup and the
// carry of the chunks before put the onsets in order.  indices [C][capacity]: the first min(count, capacity); counts [C]: all.
__global__ void __launch_bounds__(256)
trigger_onsets_kernel(const int *__restrict__ last_seen, int Bp, int lgL, int64_t N, int64_t Lat, int64_t n_samples,
                      int64_t *__restrict__ indices, int64_t capacity, int64_t *__restrict__ counts)
{
    __shared__ int buf[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int *row = last_seen + (int64_t)c * Bp;
    int64_t *idx = indices + (int64_t)c * capacity;
    const int64_t carry = trigger_onsets_row(row, Bp, lgL, N, Lat, n_samples, idx, capacity, buf, tid);
    if (tid == 0) counts[c] = carry;
}

int log2_of(int L)
{
    int lg = 0;
    while ((1 << lg) < L) lg++;
    return lg;
}

bool trigger_geometry_ok(int64_t n_evals, int C, int L, int64_t N, int64_t Lat, int64_t n_samples, int64_t first_index, int64_t hop)
{
    return n_evals >= 0 && C >= 1 && C <= 65535 && L >= 8 && L <= 4096 && (L & (L - 1)) == 0 && N >= 1 && N <= ((int64_t)1 << 24) &&
           Lat >= 0 && Lat <= ((int64_t)1 << 24) && n_samples >= 0 && first_index >= 0 && hop >= 1 && hop <= 0x7fffffffLL &&
           trigger_buffers(n_samples, L) >= 0;
}

}  // namespace

int64_t trigger_buffers(int64_t n_samples, int L)
{
    if (n_samples < 0 || L < 1) return -1;
    const int64_t Bp = (n_samples + 2 * (int64_t)L - 2) / L;           // ceil((n_samples + L - 1) / L)
    return Bp <= 0x7fffffffLL - kScanChunk ? std::max<int64_t>(Bp, 1) : -1;
}

hipError_t launch_trigger_scan(const uint8_t *flags, int64_t n_evals, int C, int L, int64_t n_samples, int64_t first_index, int64_t hop,
                               int *last_seen, hipStream_t stream)
{
    if (!trigger_geometry_ok(n_evals, C, L, 1, 0, n_samples, first_index, hop) || !last_seen || (n_evals > 0 && !flags)) return hipErrorInvalidValue;
    const int Bp = (int)trigger_buffers(n_samples, L);
    hipLaunchKernelGGL(trigger_scan_kernel, dim3((unsigned)C), dim3(256), 0, stream, flags, n_evals, first_index, hop, log2_of(L), last_seen, Bp);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_trigger_t(const int *last_seen, int C, int L, int64_t N, int64_t Lat, T *track, int64_t n_samples, int64_t stride,
                                   hipStream_t stream)
{
    if (n_samples <= 0 || C <= 0) return hipSuccess;
    if (!trigger_geometry_ok(0, C, L, N, Lat, n_samples, 0, 1) || !last_seen || !track || (C > 1 && stride < n_samples) ||
        (reinterpret_cast<uintptr_t>(track) & (sizeof(T) - 1)) != 0)
        return hipErrorInvalidValue;
    const int span = kTrigSpanBytes / (int)sizeof(T);
    const int64_t blocks = (n_samples + span - 1) / span + 1;         // (one more where a row's head shifts the spans)
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(trigger_kernel<T>, dim3((unsigned)blocks, (unsigned)C), dim3(256), 0, stream, last_seen, (int)trigger_buffers(n_samples, L),
                       track, n_samples, stride, log2_of(L), N, Lat, span);
    return hipGetLastError();
}

hipError_t launch_trigger(const int *last_seen, int C, int L, int64_t N, int64_t Lat, float *track, int64_t n_samples, int64_t stride,
                          hipStream_t stream)
{
    return launch_trigger_t<float>(last_seen, C, L, N, Lat, track, n_samples, stride, stream);
}

hipError_t launch_trigger_s16(const int *last_seen, int C, int L, int64_t N, int64_t Lat, int16_t *track, int64_t n_samples, int64_t stride,
                              hipStream_t stream)
{
    return launch_trigger_t<int16_t>(last_seen, C, L, N, Lat, track, n_samples, stride, stream);
}

hipError_t launch_trigger_interleaved_s16(const int *last_seen, int C, int L, int64_t N, int64_t Lat, const int16_t *samples,
                                          int64_t sample_stride, int16_t *frames, int64_t n_frames, hipStream_t stream)
{
    if (n_frames <= 0 || C <= 0) return hipSuccess;
    // one channel without audio: the frame-major buffer is the planar row
    if (C == 1 && !samples) return launch_trigger_s16(last_seen, 1, L, N, Lat, frames, n_frames, n_frames, stream);
    if (!trigger_geometry_ok(0, C, L, N, Lat, n_frames, 0, 1) || !last_seen || !frames || (reinterpret_cast<uintptr_t>(frames) & 1) != 0 ||
        (samples && ((C > 1 && sample_stride < n_frames) || (reinterpret_cast<uintptr_t>(samples) & 1) != 0)))
        return hipErrorInvalidValue;
    const int64_t tiles = (n_frames + kTrigTileFrames - 1) / kTrigTileFrames;
    const int ctiles = (C + kTrigTileCh - 1) / kTrigTileCh;
    if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
    const int Bp = (int)trigger_buffers(n_frames, L);
    if (samples)
        hipLaunchKernelGGL(trigger_interleaved_s16_kernel<true>, dim3((unsigned)tiles, (unsigned)ctiles), dim3(256), 0, stream, last_seen, Bp,
                           samples, sample_stride, frames, n_frames, C, log2_of(L), N, Lat);
    else
        hipLaunchKernelGGL(trigger_interleaved_s16_kernel<false>, dim3((unsigned)tiles, (unsigned)ctiles), dim3(256), 0, stream, last_seen, Bp,
                           samples, sample_stride, frames, n_frames, C, log2_of(L), N, Lat);
    return hipGetLastError();
}

hipError_t launch_trigger_onsets(const int *last_seen, int C, int L, int64_t N, int64_t Lat, int64_t n_samples, int64_t *indices,
                                 int64_t capacity, int64_t *counts, hipStream_t stream)
{
    if (C <= 0) return hipSuccess;
    if (!trigger_geometry_ok(0, C, L, N, Lat, n_samples, 0, 1) || !last_seen || !counts || capacity < 0 || (capacity > 0 && !indices))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(trigger_onsets_kernel, dim3((unsigned)C), dim3(256), 0, stream, last_seen, (int)trigger_buffers(n_samples, L), log2_of(L), N,
                       Lat, n_samples, indices, capacity, counts);
    return hipGetLastError();
}

}  // namespace sd
