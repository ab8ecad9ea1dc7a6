// hopk_schedule.hpp -- the fold kernel's sample ring at a compile-time hop (kernels_fused_s.hip, HOP = 132): which chunks a tile
// issues, the slots they land in, where the mirror copy is due.  Plain constexpr arithmetic, no device code: the kernel unrolls
// its loop over these tables, fused_plan.cpp sizes the ring by them, and tests/cpp/hopk_schedule_test.cpp walks them on the host.
//
// hop 132 (the network's windowOverlap in the reference's sample.txt), 16 frames a tile, 256-sample frames, chunks of 256 floats:
// a tile moves on by 2112 samples = 8.25 chunks, so FOUR tiles are exactly 33 chunks, and a ring of ELEVEN slots closes with that
// period (33 = 3 x 11): over four tiles every chunk number, slot, mirror copy and frame offset is a constant of the instruction
// stream.
//
//   phase | tile's chunks | issued while it runs (for the next tile) | slots          | mirror with
//     0   |   0 ..  8     |   9 .. 16                                | 9 10 0 1 .. 5  | 11
//     1   |   8 .. 16     |  17 .. 25                                | 6 .. 10 0 .. 3 | 22
//     2   |  16 .. 25     |  26 .. 33                                | 4 .. 10 0      | 33
//     3   |  24 .. 33     |  34 .. 41  (= 1 .. 8 of the next period) | 1 .. 8         | --
// (chunk numbers relative to the period's first chunk; the prologue issues 0 .. 8 of the first period, chunk 0 with its mirror)
#pragma once

namespace sd {
namespace hopk {

constexpr int kHop = 132;                 // samples between frames
constexpr int kTileFrames = 16;           // frames per wave and tile (kFusedSTileFrames)
constexpr int kWindow = 256;              // samples a frame
constexpr int kChunk = 256;               // floats a chunk (1024 bytes: one LDS-DMA instruction of a wave)
constexpr int kRing = 11;                 // slots of the ring (+ one mirror chunk behind them)
constexpr int kPeriod = 4;                // tiles after which the schedule repeats
constexpr int kPeriodChunks = 33;         // chunks a period
constexpr int kTileAdvance = kTileFrames * kHop;                     // 2112 samples
constexpr int kSpan = (kTileFrames - 1) * kHop + kWindow;            // 2236 samples under one tile
constexpr int kRingFloats = kRing * kChunk;

static_assert(kPeriod * kTileAdvance == kPeriodChunks * kChunk, "the period is a whole number of chunks");
static_assert(kPeriodChunks % kRing == 0, "the slot pattern closes with the period");
static_assert(kTileAdvance <= kRingFloats && kHop % 4 == 0, "a lane's frame offset stays inside the ring, on a quad");

// phase ph (0 .. kPeriod; kPeriod is phase 0 of the next period), chunk numbers relative to the period's first chunk
constexpr int first_chunk(int ph) { return (kTileAdvance * ph) / kChunk; }               // the first chunk tile ph reads
constexpr int last_chunk(int ph) { return (kTileAdvance * ph + kSpan - 1) / kChunk; }    // ... and the last
constexpr int issue_first(int ph) { return last_chunk(ph) + 1; }     // issued while tile ph runs, once its reads have returned:
constexpr int issue_last(int ph) { return last_chunk(ph + 1); }      //   what tile ph + 1 reads beyond tile ph
constexpr int slot_of(int q) { return q % kRing; }
constexpr bool mirrored(int q) { return q % kRing == 0; }            // slot 0's chunks are written behind the ring as well
constexpr int frame0_offset(int ph) { return (kTileAdvance * ph) % kRingFloats; }        // ring offset (floats) of the tile's first frame

// a chunk may replace the one kRing before it only if no tile still to be read needs that one: the newest chunk issued for tile
// ph + 1 replaces a chunk in front of that tile's first
constexpr bool phase_fits(int ph) { return issue_last(ph) - kRing < first_chunk(ph + 1) && last_chunk(ph) - first_chunk(ph) < kRing; }
static_assert(phase_fits(0) && phase_fits(1) && phase_fits(2) && phase_fits(3), "eleven slots hold a tile's span and the next tile's chunks");
static_assert(last_chunk(kPeriod) == last_chunk(0) + kPeriodChunks && first_chunk(kPeriod) == kPeriodChunks, "phase 4 is phase 0, one period on");

}  // namespace hopk
}  // namespace sd
