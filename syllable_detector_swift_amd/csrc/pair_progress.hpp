// pair_progress.hpp -- the fold kernel's progress words (kernels_fused_s.hip, HOP = 132): where, in a wave's share of the LDS, the
// word sits in which the wave publishes the tile it is on, and which wave reads it.  Plain constexpr arithmetic, no device code:
// the kernel addresses the words by it, its launcher refuses a plan they do not fit, and tests/cpp/pair_progress_test.cpp walks
// the layout on the host.
//
// A workgroup of the form is eight waves, two on each SIMD of its CU: wave w and wave w ^ 4 (profiles/pairstep_skew_before.txt).
// Nothing makes the two of a pair wait for each other, and at equal priority the SIMD's arbiter favours the older one, tile after
// tile -- so each wave tells its partner how far it is, and the one that is behind runs at priority 1 (kernels_fused_s.hip).
//
// A wave's share, HOP form (bytes from the share's first):
//     [0, 12288)                    the ring of eleven chunks and the mirror chunk
//     [12288, 12288 + 4 n)          n = (T - 1 + 16) pstride floats of tap-product rows,
//                                   8 floats: the zero quad and the quad for stores that have no place,
//                                   128 floats: the table of lane-group constants (zeroed with the rows; used by wider forms)
//     [share - 16, share - 12)      the progress word (the share's last quad: 16-byte aligned, behind everything above)
#pragma once

#include "hopk_schedule.hpp"

namespace sd {
namespace pairp {

constexpr int kWaves = 8;                                   // waves a workgroup of the form
constexpr int kRingBytes = (hopk::kRing + 1) * 1024;        // ring + mirror

constexpr int partner_of(int wave) { return wave ^ (kWaves / 2); }          // the other wave on this wave's SIMD

// byte offsets inside a wave's share of `share` bytes, for timeRange T and rows of `pstride` floats
constexpr int rows_begin() { return kRingBytes; }
constexpr int rows_end(int T, int pstride) { return rows_begin() + (T - 1 + hopk::kTileFrames) * pstride * 4; }
constexpr int zquads_end(int T, int pstride) { return rows_end(T, pstride) + 8 * 4; }
constexpr int table_end(int T, int pstride) { return zquads_end(T, pstride) + 128 * 4; }   // all the prologue zeroes ends here
constexpr int word_offset(int share) { return share - 16; }

// the word of wave `wave`, from the workgroup's first LDS byte
constexpr int word_address(int wave, int share) { return wave * share + word_offset(share); }

// the plan leaves the word alone: it lies inside the share, on a word, behind ring, mirror, rows, zero quads and table
constexpr bool fits(int T, int pstride, int share)
{
    return share % 4 == 0 && word_offset(share) >= table_end(T, pstride) && word_offset(share) + 4 <= share;
}

}  // namespace pairp
}  // namespace sd
