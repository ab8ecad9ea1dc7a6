// kernels_recordings.hip -- many recordings of different lengths through one bank (syldet_recordings_* of include/syldet.h).
// The reference's tool opens one file after another and runs its tracks alone (SyllableDetectorCLI/main.swift:63-130); here the
// recordings lie end to end in the bank's rows, each from a multiple of hop, and go through the batch kernels unchanged.
//
//   recordings_load_kernel     the rows: every element [0, row_samples) of every row is a recording's sample or +0 (the pads
//                              behind each recording, the tail of shorter rows); the gather is also the de-interleave of a
//                              multi-track file (sample i of a slot is src[src_offset + i src_step])
//   recordings_events_kernel   each recording's debounced detections and their outputs out of the packed flags: one wave a
//                              recording, the scan of detections_kernel (detections_scan.hpp) from the recording's first
//                              evaluation with debounceUntil = -1; evaluations between two recordings are never read
//
// gfx950 only: wave = 64 lanes, 256-thread workgroups.

#include "detections_scan.hpp"
#include "kernels.hpp"

namespace sd {

namespace {

constexpr int kBlock = 256;
constexpr int kWave = 64;

// 16 bytes of a row as G elements
template <typename T, int G>
struct alignas(sizeof(T) * G) Group {
    T v[G];
};

// The group of G elements at row position p (a multiple of G).  s: a slot of the row that starts at or before p (the tile's).
// Wide where the group lies inside one recording whose samples are contiguous (16, 8 or 4 bytes an access, as its source address
// allows); else element by element (a group may hold the end of one recording, its pad and the start of the next: hop may be odd).
template <typename T, int G>
__device__ __forceinline__ Group<T, G> gather(const RecSlotDev *__restrict__ slots, int s, int se, const T *__restrict__ src,
                                              bool src_wide, int64_t p)
{
    Group<T, G> g;
#pragma unroll
    for (int i = 0; i < G; i++) g.v[i] = (T)0;
    if (s >= se) return g;                                        // a row without a recording
    while (s + 1 < se && slots[s + 1].offset <= p) s++;
    const RecSlotDev sl = slots[s];
    const int64_t rel = p - sl.offset;
    if constexpr (G > 1) if (src_wide && sl.src_step == 1 && rel + G <= sl.n_samples) {
        // contiguous samples: as wide as their address allows (rows start at multiples of hop: with hop 132 every second int16
        // recording is 8 bytes off a whole 16)
        const T *at = src + sl.src_offset + rel;
        const unsigned off = (unsigned)((sl.src_offset + rel) * (int64_t)sizeof(T)) & 15u;
        union { Group<T, G> g; uint4 q; uint2 d[2]; unsigned w[4]; } u;
        if (off == 0) {
            u.q = *reinterpret_cast<const uint4 *>(at);
            return u.g;
        }
        if ((off & 7u) == 0) {
            u.d[0] = reinterpret_cast<const uint2 *>(at)[0];
            u.d[1] = reinterpret_cast<const uint2 *>(at)[1];
            return u.g;
        }
        if ((off & 3u) == 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) u.w[i] = reinterpret_cast<const unsigned *>(at)[i];
            return u.g;
        }
    }
    if (rel >= sl.n_samples && (s + 1 >= se || slots[s + 1].offset >= p + G)) return g;   // all of it in a pad
    RecSlotDev cur = sl;
#pragma unroll
    for (int i = 0; i < G; i++) {
        const int64_t q = p + i;
        while (s + 1 < se && slots[s + 1].offset <= q) cur = slots[++s];
        const int64_t r = q - cur.offset;
        if (r < cur.n_samples) g.v[i] = src[cur.src_offset + r * (int64_t)cur.src_step];
    }
    return g;
}

// grid (tiles, C): workgroup (t, c) writes samples [t kRecTile, (t + 1) kRecTile) of row c, G elements (16 bytes where the rows
// allow it, else one element) a lane and access, up to four accesses a lane in flight.
template <typename T, int G>
__global__ void __launch_bounds__(kBlock)
recordings_load_kernel(RecLoadDesc d, const T *__restrict__ src, bool src_wide, T *__restrict__ rows, int64_t stride)
{
    constexpr int kPer = kRecTile / G / kBlock;                   // accesses a lane
    constexpr int kBatch = 4;
    static_assert(kPer % kBatch == 0, "a tile is whole batches");
    const int c = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * kRecTile;
    const int se = d.row_begin[c + 1];
    const int s0 = d.tile_first[(int64_t)c * d.tiles + blockIdx.x];
    T *row = rows + (int64_t)c * stride;
    for (int it = 0; it < kPer; it += kBatch) {
        Group<T, G> g[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; b++) {
            const int64_t p = t0 + ((int64_t)(it + b) * kBlock + threadIdx.x) * G;
            if (p < d.row_samples) g[b] = gather<T, G>(d.slots, s0, se, src, src_wide, p);
        }
#pragma unroll
        for (int b = 0; b < kBatch; b++) {
            const int64_t p = t0 + ((int64_t)(it + b) * kBlock + threadIdx.x) * G;
            if (p < d.row_samples) *reinterpret_cast<Group<T, G> *>(row + p) = g[b];
        }
    }
}

// One wave a recording: detections_kernel's scan over the recording's own flags (row `row` from first_eval on), sample numbers
// counted from the recording's start; detection i also carries the n_out outputs of its evaluation.
__global__ void __launch_bounds__(kWave)
recordings_events_kernel(const RecEventDev *__restrict__ desc, int64_t row_evals, int n_out, const float *__restrict__ outputs,
                         const uint8_t *__restrict__ flags, int64_t first_index, int64_t hop, int64_t debounce_frames,
                         int64_t *__restrict__ indices, float *__restrict__ values, int64_t capacity, int64_t *__restrict__ counts)
{
    const int k = blockIdx.x;
    const int lane = threadIdx.x;
    const RecEventDev d = desc[k];
    const int64_t base = (int64_t)d.row * row_evals + d.first_eval;
    int64_t *out = indices ? indices + (int64_t)k * capacity : nullptr;
    const int64_t n = debounce_scan(flags + base, d.n_evals, first_index, hop, debounce_frames, lane, [&](int64_t i, int64_t e, int64_t hit) {
        if (i >= capacity) return;
        if (lane == 0 && out) out[i] = hit;
        if (values)
            for (int o = lane; o < n_out; o += kWave) values[((int64_t)k * capacity + i) * n_out + o] = outputs[(base + e) * n_out + o];
    });
    if (lane == 0 && counts) counts[k] = n;
}

template <typename T>
hipError_t load_as(const RecLoadDesc &d, const void *src, void *rows, int64_t stride, int C, hipStream_t stream)
{
    constexpr int G = 16 / (int)sizeof(T);
    const dim3 grid((unsigned)d.tiles, (unsigned)C);
    const bool dst_wide = ((uintptr_t)rows & 15) == 0 && ((stride * (int64_t)sizeof(T)) & 15) == 0;
    const bool src_wide = ((uintptr_t)src & 15) == 0;
    if (dst_wide)
        hipLaunchKernelGGL((recordings_load_kernel<T, G>), grid, dim3(kBlock), 0, stream, d, (const T *)src, src_wide, (T *)rows, stride);
    else
        hipLaunchKernelGGL((recordings_load_kernel<T, 1>), grid, dim3(kBlock), 0, stream, d, (const T *)src, false, (T *)rows, stride);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_recordings_load(const RecLoadDesc &d, const void *src, bool s16, void *rows, int64_t stride, int C, hipStream_t stream)
{
    if (C <= 0 || d.tiles <= 0) return hipSuccess;
    return s16 ? load_as<int16_t>(d, src, rows, stride, C, stream) : load_as<float>(d, src, rows, stride, C, stream);
}

hipError_t launch_recordings_events(const RecEventDev *desc, int K, int64_t row_evals, int n_out, const float *outputs, const uint8_t *flags,
                                    int64_t first_index, int64_t hop, int64_t debounce_frames, int64_t *indices, float *values,
                                    int64_t capacity, int64_t *counts, hipStream_t stream)
{
    if (K <= 0) return hipSuccess;
    hipLaunchKernelGGL(recordings_events_kernel, dim3((unsigned)K), dim3(kWave), 0, stream, desc, row_evals, n_out, outputs, flags,
                       first_index, hop, debounce_frames, indices, values, capacity, counts);
    return hipGetLastError();
}

}  // namespace sd
