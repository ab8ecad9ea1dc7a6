// kernels_recordings_tracks.hip -- the two per-sample tracks of packed recordings (syldet_recordings_trace_device*,
// syldet_recordings_trigger*_device* of include/syldet.h): every recording of a packed bank gets the Simulator's output track
// (kernels_trace.hip) and the TTL trigger track (kernels_trigger.hip) it would have had alone, written straight to a destination
// of its own -- element i of recording k goes to dst[dst_offset[k] + i dst_step[k]] -- in a fixed number of launches whatever K is.
//
//   recordings_hold_kernel<T>             outputs [C][row_evals][n_out] -> every recording's trace; syldet_timings lists it as
//                                         "recordings_trace_kernel" (the symbol has another name because the build's ISA check of
//                                         kernels_trace.hip finds that file by the text of its kernel's name)
//   recordings_trigger_scan_kernel        flags [C][row_evals] -> every recording's last_seen table, the tables end to end
//   recordings_trigger_kernel<T>          the tables -> every recording's trigger track
//   recordings_trigger_onsets_kernel      the tables -> every recording's rising edges, in order
//
// The values are those of the one-recording kernels (track_values.hpp states each once); what differs is where a recording
// begins.  Sample i of a recording at row offset o lies at row position p = o + i, and o is a multiple of hop, so the recording's
// evaluation e is row evaluation o / hop + e: everything below counts i, e and the buffers b(e) = (D + e hop - 1) / L from the
// recording's own start, and masks what lies outside it (i < D, e >= n_evals, i >= n_samples), so that neither a hold nor a
// pulse reaches the next recording of the row.
//
// The expansion kernels are balanced by ROWS, not by recordings (lengths differ by orders of magnitude): workgroup (t, c) takes
// the row positions [t kRecTile, (t + 1) kRecTile) of row c -- the load's tiles, and its tile_first table -- and walks the slots
// that cross them.  For each slot it puts the evaluations (the table entries) its part of the recording asks for into LDS, then
// stores: where dst_step is 1, 16 bytes a lane in groups aligned to the DESTINATION, the part's head and tail element by
// element; element by element for any other step.  The scan and the onsets are one workgroup a recording with the chunk walk of
// trigger_scan_kernel: no workgroup waits for another one, so nothing can spin.
//
// Compiled like kernels_trace.hip and kernels_trigger.hip: -ffp-contract=off, no fast-math flag (see the Makefile) -- the trace's
// `/` is the correctly rounded fp32 division and its product with 32767 rounds on its own, here as there.
//
// gfx950 only.  wave = 64.  Every value is written with ordinary vector stores.

#include "kernels.hpp"
#include "track_values.hpp"

namespace sd {

namespace {

constexpr int kBlock = 256;
constexpr int kTrackEvals = kRecTile + 16;     // evaluations a tile's part of a recording may touch (hop 1: one a sample, and one more)
constexpr int kTrackSlice = kRecTile / 8 + 8;  // table entries it may touch (L = 8: one for eight samples, and two more)

// The part [iA, iB) of one recording's elements that a tile holds, stored through `one` (the word of element i) and `group` (the
// words of the G elements from i on).  Uniform over the workgroup but for the lane's share.
template <typename T, class One, class Group>
__device__ __forceinline__ void store_part(T *__restrict__ dst, const RecTrackDev tr, int64_t iA, int64_t iB, int tid, One one, Group group)
{
    constexpr bool S16 = sizeof(T) == 2;
    constexpr int G = 16 / (int)sizeof(T);
    auto put = [&](int64_t at, unsigned w) {
        if (S16) reinterpret_cast<uint16_t *>(dst)[at] = (uint16_t)w;
        else reinterpret_cast<unsigned *>(dst)[at] = w;
    };
    if (tr.dst_step != 1) {
        for (int64_t i = iA + tid; i < iB; i += kBlock) put(tr.dst_offset + i * (int64_t)tr.dst_step, one(i));
        return;
    }
    T *base = dst + tr.dst_offset;                                       // element i at base[i]
    const int64_t off = (int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(base + iA) & 15u)) & 15u) / (int64_t)sizeof(T);
    const int head = (int)min(off, iB - iA);
    const int64_t gA = iA + head;                                        // the first aligned group
    const int64_t groups = (iB - gA) / G;
    const int64_t tA = gA + groups * G;                                  // the tail: fewer than G elements
    if (tid < head) put(tr.dst_offset + iA + tid, one(iA + tid));
    if (tid >= 64 && tA + (tid - 64) < iB) put(tr.dst_offset + tA + (tid - 64), one(tA + (tid - 64)));
    for (int64_t g = tid; g < groups; g += kBlock) {
        const int64_t i = gA + g * G;
        unsigned w[G];
        group(i, w);
        uint4 v;
        if (S16) v = make_uint4(w[0] | (w[1] << 16), w[2] | (w[3] << 16), w[4] | (w[5] << 16), w[6] | (w[7] << 16));
        else v = make_uint4(w[0], w[1], w[2], w[3]);
        *reinterpret_cast<uint4 *>(base + i) = v;
    }
}

// The slots of row c that cross tile t, one after another: part(slot, track, iA, iB) is called by the whole workgroup.
template <class Part>
__device__ __forceinline__ void walk_tile(const RecTrackDesc &d, Part part)
{
    const int c = blockIdx.y;
    const int64_t p0 = (int64_t)blockIdx.x * kRecTile, p1 = min(p0 + (int64_t)kRecTile, d.load.row_samples);
    const int se = d.load.row_begin[c + 1];
    for (int s = d.load.tile_first[(int64_t)c * d.load.tiles + blockIdx.x]; s < se; s++) {
        const RecSlotDev sl = d.load.slots[s];
        if (sl.offset >= p1) break;
        const int64_t iA = max(p0 - sl.offset, (int64_t)0), iB = min(p1 - sl.offset, sl.n_samples);
        if (iA >= iB) continue;                                          // (a pad, or a recording without samples)
        part(d.dst[s], iA, iB);
    }
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
recordings_hold_kernel(RecTrackDesc d, const float *__restrict__ outputs, int n_out, int k, const float *__restrict__ thr, T *__restrict__ dst,
                        int64_t D, unsigned hop, unsigned hop_magic)
{
    constexpr bool S16 = sizeof(T) == 2;
    constexpr int G = 16 / (int)sizeof(T);
    __shared__ unsigned ev[kTrackEvals];
    const int c = blockIdx.y, tid = threadIdx.x;
    const float t = thr[c];
    walk_tile(d, [&](const RecTrackDev tr, int64_t iA, int64_t iB) {
        const RecEventDev rec = d.events[tr.k];
        // the evaluations [eA, eA + nE) of the recording that its elements [iA, iB) hold: the one full division of the part
        const int64_t first = max(iA, D);
        const int64_t eA = (first - D) / (int64_t)hop;
        const int64_t base = D + eA * (int64_t)hop;                      // first sample of evaluation eA: first - hop < base <= first
        const int nE = iB > D ? (int)div_magic((unsigned)(iB - 1 - base), hop, hop_magic) + 1 : 0;
        const float *row = outputs + ((int64_t)c * d.row_evals + rec.first_eval) * n_out + k;
        __syncthreads();                                                 // (the slot before has been stored)
        for (int i = tid; i < nE; i += kBlock) ev[i] = trace_word<S16>(row, eA + i, rec.n_evals, n_out, t);
        __syncthreads();
        auto one = [&](int64_t i) { return i < D ? 0u : ev[div_magic((unsigned)(i - base), hop, hop_magic)]; };
        auto group = [&](int64_t i, unsigned *w) {
            const int64_t rel = i - base;                                // negative only in front of D (base is D there)
            const int lead = rel < 0 ? (int)min((int64_t)G, -rel) : 0;
            const unsigned r = rel < 0 ? 0u : (unsigned)rel;
            unsigned e = div_magic(r, hop, hop_magic), rem = r - e * hop;
#pragma unroll
            for (int j = 0; j < G; j++) {
                const bool live = j >= lead;
                w[j] = live ? ev[e] : 0u;
                if (live && ++rem == hop) { rem = 0; e++; }
            }
        };
        store_part(dst, tr, iA, iB, tid, one, group);
    });
}

// One workgroup a recording: trigger_scan_kernel on the recording's own flags, into its own table.
__global__ void __launch_bounds__(kBlock)
recordings_trigger_scan_kernel(RecTrackDesc d, const uint8_t *__restrict__ flags, int64_t D, int64_t hop, int lgL, int *__restrict__ last_seen)
{
    __shared__ int seen[kScanChunk];
    __shared__ int buf[256];
    const int k = blockIdx.x;
    const RecEventDev rec = d.events[k];
    const int at = d.ls_begin[k];
    trigger_scan_row(flags + (int64_t)rec.row * d.row_evals + rec.first_eval, rec.n_evals, D, hop, lgL, last_seen + at, d.ls_begin[k + 1] - at,
                     seen, buf, threadIdx.x);
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
recordings_trigger_kernel(RecTrackDesc d, const int *__restrict__ last_seen, T *__restrict__ dst, int lgL, int64_t N, int64_t Lat)
{
    constexpr bool S16 = sizeof(T) == 2;
    constexpr int G = 16 / (int)sizeof(T);
    constexpr unsigned kHigh = S16 ? 32767u : 0x3f800000u;               // 32767, or the bits of 1.0f
    __shared__ int ls[kTrackSlice];
    const int tid = threadIdx.x;
    const int64_t L = (int64_t)1 << lgL;
    walk_tile(d, [&](const RecTrackDev tr, int64_t iA, int64_t iB) {
        // table entries [qA, qA + nQ) of the part (clamped to the recording's table)
        const int64_t qA = iA - Lat >= L ? ((iA - Lat) >> lgL) - 1 : 0;
        const int64_t qB = iB - 1 - Lat >= L ? ((iB - 1 - Lat) >> lgL) - 1 : -1;
        const int nQ = qB >= qA ? (int)min(qB - qA + 1, (int64_t)kTrackSlice) : 0;
        const int at0 = d.ls_begin[tr.k];
        const int Bp = d.ls_begin[tr.k + 1] - at0;
        __syncthreads();                                                 // (the slot before has been stored)
        for (int i = tid; i < nQ; i += kBlock) ls[i] = last_seen[at0 + (int)min(qA + i, (int64_t)Bp - 1)];
        __syncthreads();
        auto at = [&](int64_t q) { return ls[min(max(q - qA, (int64_t)0), (int64_t)(kTrackSlice - 1))]; };
        auto one = [&](int64_t i) { return (nQ > 0 && trigger_high(i, Lat, lgL, N, at)) ? kHigh : 0u; };
        auto group = [&](int64_t i, unsigned *w) {
#pragma unroll
            for (int j = 0; j < G; j++) w[j] = one(i + j);
        };
        store_part(dst, tr, iA, iB, tid, one, group);
    });
}

// One workgroup a recording: trigger_onsets_kernel on the recording's own table.  indices [K][capacity], counts [K].
__global__ void __launch_bounds__(kBlock)
recordings_trigger_onsets_kernel(RecTrackDesc d, const int *__restrict__ last_seen, int lgL, int64_t N, int64_t Lat,
                                 int64_t *__restrict__ indices, int64_t capacity, int64_t *__restrict__ counts)
{
    __shared__ int buf[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    const int at = d.ls_begin[k];
    const int64_t n = trigger_onsets_row(last_seen + at, d.ls_begin[k + 1] - at, lgL, N, Lat, d.n_samples[k], indices + (int64_t)k * capacity,
                                         capacity, buf, tid);
    if (tid == 0) counts[k] = n;
}

int log2_of(int L)
{
    int lg = 0;
    while ((1 << lg) < L) lg++;
    return lg;
}

bool trigger_ok(int L, int64_t N, int64_t Lat)
{
    return L >= 8 && L <= 4096 && (L & (L - 1)) == 0 && N >= 1 && N <= ((int64_t)1 << 24) && Lat >= 0 && Lat <= ((int64_t)1 << 24);
}

}  // namespace

hipError_t launch_recordings_trace(const RecTrackDesc &d, int C, const float *outputs, int n_out, int k, const float *thr, void *dst, bool s16,
                                   int64_t first_index, int64_t hop, hipStream_t stream)
{
    if (C <= 0 || d.K <= 0 || d.load.tiles <= 0) return hipSuccess;
    if (hop < 1 || hop > 0x7fffffffLL - 2 * kRecTile || first_index < 0 || n_out < 1 || k < 0 || k >= n_out || C > 65535 || !dst || !thr ||
        (d.row_evals > 0 && !outputs) || (reinterpret_cast<uintptr_t>(dst) & (s16 ? 1u : 3u)) != 0)
        return hipErrorInvalidValue;
    const unsigned magic = magic_for((uint64_t)kRecTile + 16 + (uint64_t)hop, (unsigned)hop);
    const dim3 grid((unsigned)d.load.tiles, (unsigned)C);
    if (s16)
        hipLaunchKernelGGL(recordings_hold_kernel<int16_t>, grid, dim3(kBlock), 0, stream, d, outputs, n_out, k, thr, (int16_t *)dst, first_index,
                           (unsigned)hop, magic);
    else
        hipLaunchKernelGGL(recordings_hold_kernel<float>, grid, dim3(kBlock), 0, stream, d, outputs, n_out, k, thr, (float *)dst, first_index,
                           (unsigned)hop, magic);
    return hipGetLastError();
}

hipError_t launch_recordings_trigger_scan(const RecTrackDesc &d, const uint8_t *flags, int L, int64_t first_index, int64_t hop, int *last_seen,
                                          hipStream_t stream)
{
    if (d.K <= 0) return hipSuccess;
    if (!trigger_ok(L, 1, 0) || first_index < 0 || hop < 1 || hop > 0x7fffffffLL || !last_seen || (d.row_evals > 0 && !flags)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recordings_trigger_scan_kernel, dim3((unsigned)d.K), dim3(kBlock), 0, stream, d, flags, first_index, hop, log2_of(L), last_seen);
    return hipGetLastError();
}

hipError_t launch_recordings_trigger(const RecTrackDesc &d, int C, const int *last_seen, int L, int64_t N, int64_t Lat, void *dst, bool s16,
                                     hipStream_t stream)
{
    if (C <= 0 || d.K <= 0 || d.load.tiles <= 0) return hipSuccess;
    if (!trigger_ok(L, N, Lat) || C > 65535 || !last_seen || !dst || (reinterpret_cast<uintptr_t>(dst) & (s16 ? 1u : 3u)) != 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)d.load.tiles, (unsigned)C);
    if (s16) hipLaunchKernelGGL(recordings_trigger_kernel<int16_t>, grid, dim3(kBlock), 0, stream, d, last_seen, (int16_t *)dst, log2_of(L), N, Lat);
    else hipLaunchKernelGGL(recordings_trigger_kernel<float>, grid, dim3(kBlock), 0, stream, d, last_seen, (float *)dst, log2_of(L), N, Lat);
    return hipGetLastError();
}

hipError_t launch_recordings_trigger_onsets(const RecTrackDesc &d, const int *last_seen, int L, int64_t N, int64_t Lat, int64_t *indices,
                                            int64_t capacity, int64_t *counts, hipStream_t stream)
{
    if (d.K <= 0) return hipSuccess;
    if (!trigger_ok(L, N, Lat) || !last_seen || !counts || capacity < 0 || (capacity > 0 && !indices)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(recordings_trigger_onsets_kernel, dim3((unsigned)d.K), dim3(kBlock), 0, stream, d, last_seen, log2_of(L), N, Lat, indices,
                       capacity, counts);
    return hipGetLastError();
}

}  // namespace sd
