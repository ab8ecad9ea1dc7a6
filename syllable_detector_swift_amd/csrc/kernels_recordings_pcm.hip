// kernels_recordings_pcm.hip -- packed recordings from the files' own bytes (syldet_recordings_load_pcm_device of include/syldet.h):
// every recording of a plan decoded from its own little-endian sample format, de-interleaved and placed in the fp32 rows in one
// launch.  The reference has AVFoundation deliver every file as 32-bit float (audioSettings, Common/SyllableDetector.swift:19-23)
// and runs the files one after another (SyllableDetectorCLI/main.swift:63-130); the values are pcm_values.hpp's, which the host
// (syldet_pcm_decode) shares.
//
//   recordings_load_pcm_kernel   recordings_load_kernel's grid and tile walk (kernels_recordings.hip): workgroup (t, c) writes
//                                samples [t kRecTile, (t + 1) kRecTile) of row c, 16 bytes a lane and store where the rows allow,
//                                four accesses a lane in flight
//
// A wave's lanes usually lie in one recording.  Each wave takes the slots among its lanes in turn (readfirstlane on the slot index):
// the slot's entry comes through scalar loads and its format decides a scalar branch, not a switch a lane.  Four samples wholly
// inside a contiguous recording are read as wide as their address allows (pcm_group4: S16 8 bytes, S24 12, S32 and F32 16, F64 32,
// U8 4); an interleaved recording's sample by sample; a group that holds a recording's end, a pad or the next recording's start
// element by element with the lane's own slots.  No byte outside a recording's own samples is read, and no multi-byte access is
// off a multiple of its size.
//
// gfx950 only: wave = 64 lanes, 256-thread workgroups.  Compiled with -ffp-contract=off (see the Makefile).

#include "kernels.hpp"
#include "pcm_values.hpp"

namespace sd {

namespace {

constexpr int kBlock = 256;

// The handle's table through the constant address space: no launch writes it, and only so does the compiler read the wave's slot
// with scalar loads although the kernel stores (to the rows) between two reads.
typedef __attribute__((address_space(4))) const RecSlotDev *ConstSlots;

// 16 bytes of a row (G = 4), or one element
template <int G>
struct alignas(sizeof(float) * G) Quad {
    float v[G];
};

// The G elements at row position p (a multiple of G).  s: a slot of the row that starts at or before p (the tile's).
template <int G>
__device__ __forceinline__ Quad<G> gather_pcm(const RecSlotDev *__restrict__ slots, int s, int se, const unsigned char *__restrict__ src, int64_t p)
{
    Quad<G> g;
#pragma unroll
    for (int i = 0; i < G; i++) g.v[i] = 0.0f;
    if (s >= se) return g;                                        // a row without a recording
    while (s + 1 < se && slots[s + 1].offset <= p) s++;
    // the slots among the wave's lanes, one a pass: lanes leave the loop with their slot's turn
    bool mixed = false;
    for (bool waiting = true; waiting;) {
        const int su = __builtin_amdgcn_readfirstlane(s);
        // (read in front of the comparison: behind it the compiler knows s == su and reads the entry a lane instead)
        const ConstSlots ks = (ConstSlots)(uintptr_t)slots + su;
        const RecSlotDev sl{ks->offset, ks->n_samples, ks->src_offset, ks->src_step, ks->format};        // scalar loads
        if (s == su) {
            const int64_t rel = p - sl.offset;
            if (rel + G <= sl.n_samples) {
                const int size = pcm_sample_bytes(sl.format);
                const unsigned char *at = src + sl.src_offset + rel * (int64_t)sl.src_step;
                if (G == 4 && sl.src_step == size) {
                    pcm_group4(sl.format, at, g.v);
                } else {
#pragma unroll
                    for (int i = 0; i < G; i++) g.v[i] = pcm_value(sl.format, at + (int64_t)i * sl.src_step);
                }
            } else {
                mixed = rel < sl.n_samples || (su + 1 < se && slots[su + 1].offset < p + G);      // else all of it in a pad
            }
            waiting = false;
        }
    }
    if (mixed) {
        RecSlotDev cur = slots[s];
#pragma unroll
        for (int i = 0; i < G; i++) {
            const int64_t q = p + i;
            while (s + 1 < se && slots[s + 1].offset <= q) cur = slots[++s];
            const int64_t r = q - cur.offset;
            if (r < cur.n_samples) g.v[i] = pcm_value(cur.format, src + cur.src_offset + r * (int64_t)cur.src_step);
        }
    }
    return g;
}

template <int G>
__global__ void __launch_bounds__(kBlock)
recordings_load_pcm_kernel(RecLoadDesc d, const unsigned char *__restrict__ src, float *__restrict__ rows, int64_t stride)
{
    constexpr int kPer = kRecTile / G / kBlock;                   // accesses a lane
    constexpr int kBatch = 4;
    static_assert(kPer % kBatch == 0, "a tile is whole batches");
    const int c = blockIdx.y;
    const int64_t t0 = (int64_t)blockIdx.x * kRecTile;
    const int se = d.row_begin[c + 1];
    const int s0 = d.tile_first[(int64_t)c * d.tiles + blockIdx.x];
    float *row = rows + (int64_t)c * stride;
    for (int it = 0; it < kPer; it += kBatch) {
        Quad<G> g[kBatch];
#pragma unroll
        for (int b = 0; b < kBatch; b++) {
            const int64_t p = t0 + ((int64_t)(it + b) * kBlock + threadIdx.x) * G;
            if (p < d.row_samples) g[b] = gather_pcm<G>(d.slots, s0, se, src, p);
        }
#pragma unroll
        for (int b = 0; b < kBatch; b++) {
            const int64_t p = t0 + ((int64_t)(it + b) * kBlock + threadIdx.x) * G;
            if (p < d.row_samples) *reinterpret_cast<Quad<G> *>(row + p) = g[b];
        }
    }
}

}  // namespace

hipError_t launch_recordings_load_pcm(const RecLoadDesc &d, const void *src, float *rows, int64_t stride, int C, hipStream_t stream)
{
    if (C <= 0 || d.tiles <= 0) return hipSuccess;
    const dim3 grid((unsigned)d.tiles, (unsigned)C);
    const bool dst_wide = ((uintptr_t)rows & 15) == 0 && ((stride * (int64_t)sizeof(float)) & 15) == 0;
    if (dst_wide)
        hipLaunchKernelGGL(recordings_load_pcm_kernel<4>, grid, dim3(kBlock), 0, stream, d, (const unsigned char *)src, rows, stride);
    else
        hipLaunchKernelGGL(recordings_load_pcm_kernel<1>, grid, dim3(kBlock), 0, stream, d, (const unsigned char *)src, rows, stride);
    return hipGetLastError();
}

}  // namespace sd
