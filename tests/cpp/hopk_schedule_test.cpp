// The fold kernel's compile-time ring schedule (hop 132: syllable_detector_swift_amd/csrc/hopk_schedule.hpp) walked on the
// host, from the same constexpr tables the kernel is compiled from.  A wave is modelled as the kernel runs it: the prologue's
// chunks, then per tile the reads of its sixteen frames and, once they have returned, the next tile's chunks; the period's base
// moves on after phase 3.  For segments of 1 to 40 tiles:
//   * every sample a tile reads lies in a chunk that has been issued and not yet overwritten (and sits where the lane looks);
//   * no chunk is issued over a slot that a tile still to be read needs, and the chunks go out in order, none twice, none missing;
//   * the mirror holds slot 0's current chunk whenever a frame reads across the ring's end.
// CPU only; prints "ok" and exits 0, or says what broke and exits 1.
#include <cstdio>
#include <cstdlib>

#include "hopk_schedule.hpp"

using namespace sd::hopk;

namespace {

struct Wave {
    long slot[kRing];          // the chunk (counted from the segment's first sample) each ring slot holds, -1: none yet
    long mirror = -1;          // ... and the mirror chunk behind the ring
    long next = 0;             // the next chunk the stream owes
    long base = 0;             // the period's first chunk (what the kernel's per-period byte offset stands for)
    int ph = 0;                // the tile's phase
    long t_unread = 0;         // the first tile whose reads have not returned
};

[[noreturn]] void fail(int tiles, long t, const char *what, long a, long b)
{
    std::printf("segment of %d tiles, tile %ld: %s (%ld, %ld)\n", tiles, t, what, a, b);
    std::exit(1);
}

void issue(Wave &w, int tiles, long t, int qf, int ql)
{
    for (int q = qf; q <= ql; q++) {
        const long chunk = w.base + q;
        if (chunk != w.next) fail(tiles, t, "chunks out of order", chunk, w.next);
        const int s = slot_of(q);
        if (s != (int)(chunk % kRing)) fail(tiles, t, "the period's base is not a multiple of the ring", chunk, s);
        // what it replaces must be dead: in front of the first chunk of the first tile still to be read
        const long first_needed = (kTileAdvance * w.t_unread) / kChunk;
        if (w.slot[s] >= first_needed) fail(tiles, t, "a chunk replaces one that an unread tile needs", chunk, w.slot[s]);
        w.slot[s] = chunk;
        if (mirrored(q)) {
            if (s != 0) fail(tiles, t, "a mirror copy of another slot than 0", chunk, s);
            w.mirror = chunk;
        } else if (s == 0) {
            fail(tiles, t, "slot 0 written without its mirror copy", chunk, s);
        }
        w.next = chunk + 1;
    }
}

void segment(int tiles)
{
    Wave w;
    for (int s = 0; s < kRing; s++) w.slot[s] = -1;
    issue(w, tiles, -1, 0, last_chunk(0));                       // the prologue: tile 0's chunks
    long fo[kTileFrames];                                         // a lane's frame offset in the ring, advanced as the kernel does
    for (int f = 0; f < kTileFrames; f++) fo[f] = kHop * f;
    for (long t = 0; t < tiles; t++) {
        if (w.ph != (int)(t % kPeriod)) fail(tiles, t, "phase", w.ph, t % kPeriod);
        for (int f = 0; f < kTileFrames; f++) {
            if (fo[f] != (frame0_offset(w.ph) + kHop * f) % kRingFloats) fail(tiles, t, "frame offset", fo[f], f);
            const long s0 = kTileAdvance * t + kHop * f;        // the frame's first sample
            for (int i = 0; i < kWindow; i++) {
                const long smp = s0 + i, p = fo[f] + i;
                if (smp / kChunk >= w.next) fail(tiles, t, "a sample of a chunk not yet issued", smp, w.next);
                if (p < kRingFloats) {
                    if (w.slot[p / kChunk] != smp / kChunk || p % kChunk != smp % kChunk) fail(tiles, t, "the slot holds another chunk", smp, w.slot[p / kChunk]);
                } else {
                    if (p - kRingFloats >= kChunk) fail(tiles, t, "a read beyond the mirror", smp, p);
                    if (w.mirror != smp / kChunk || (p - kRingFloats) != smp % kChunk) fail(tiles, t, "the mirror holds another chunk", smp, w.mirror);
                    if (w.slot[0] != w.mirror) fail(tiles, t, "the mirror is not slot 0's current chunk", w.slot[0], w.mirror);
                }
            }
        }
        w.t_unread = t + 1;
        if (t + 1 < tiles) {                                     // the next tile's chunks, once this tile's reads have returned
            issue(w, tiles, t, issue_first(w.ph), issue_last(w.ph));
            if (w.ph == kPeriod - 1) w.base += kPeriodChunks;
            if (w.next - 1 != (kTileAdvance * (t + 1) + kSpan - 1) / kChunk) fail(tiles, t, "the next tile's last chunk is not the last issued", w.next - 1, t + 1);
        }
        for (int f = 0; f < kTileFrames; f++) {
            fo[f] += kTileAdvance;
            if (fo[f] >= kRingFloats) fo[f] -= kRingFloats;
        }
        w.ph = (w.ph + 1) & (kPeriod - 1);
    }
}

}  // namespace

int main()
{
    for (int tiles = 1; tiles <= 40; tiles++) segment(tiles);
    std::printf("ok\n");
    return 0;
}
