// The fold kernel's progress words (csrc/pair_progress.hpp) walked on the host: for every timeRange the form takes (1 .. 12) and the
// layout its plan gives a wave's share of the LDS at hop 132 -- eleven ring chunks and the mirror, the rows of tap products, the
// zero quads, the lane-group table -- the eight words are distinct, on a word, inside their wave's share and outside every one of
// those regions, and a wave's partner is the wave four on whose partner it is.  No GPU.
#include <cstdio>
#include <set>

#include "pair_progress.hpp"

using namespace sd;

namespace {

constexpr int kShare = 160 * 1024 / pairp::kWaves;        // a wave's share of the workgroup's LDS (fused_plan.cpp: per_wave)

// rows of tap products: an even number of taps a row, four products a tap, a quad of statistics (fused_plan.cpp: PSs at one quad of units)
int pstride_of(int T) { return 4 * ((T + 1) / 2 * 2) + 4; }

struct Region {
    const char *name;
    int begin, end;
};

int fail(const char *what, int T, int wave)
{
    std::printf("timeRange %d, wave %d: %s\n", T, wave, what);
    return 1;
}

}  // namespace

int main()
{
    static_assert(pairp::kWaves == 8, "two waves on each of four SIMDs");
    for (int w = 0; w < pairp::kWaves; w++) {
        const int p = pairp::partner_of(w);
        if (p == w || p < 0 || p >= pairp::kWaves || pairp::partner_of(p) != w || (p & 3) != (w & 3)) return fail("the partner is not the SIMD's other wave", 0, w);
    }
    for (int T = 1; T <= 12; T++) {
        const int ps = pstride_of(T);
        if (!pairp::fits(T, ps, kShare)) return fail("the launcher would refuse the plan", T, -1);
        // a layout whose rows reach the word must be refused
        if (pairp::fits(T, ps, pairp::table_end(T, ps) + 12) || !pairp::fits(T, ps, pairp::table_end(T, ps) + 16)) return fail("fits() does not guard the word", T, -1);
        const Region regions[] = {
            {"ring", 0, hopk::kRing * 1024},
            {"mirror", hopk::kRing * 1024, (hopk::kRing + 1) * 1024},
            {"rows", pairp::rows_begin(), pairp::rows_end(T, ps)},
            {"zero quads", pairp::rows_end(T, ps), pairp::zquads_end(T, ps)},
            {"lane-group table", pairp::zquads_end(T, ps), pairp::table_end(T, ps)},
        };
        // the regions are what the kernel lays out: (T - 1 + 16) rows of ps floats, 8 floats, 128 floats, back to back behind the mirror
        if (regions[2].begin != regions[1].end || regions[2].end - regions[2].begin != (T - 1 + hopk::kTileFrames) * ps * 4 ||
            regions[3].end - regions[3].begin != 32 || regions[4].end - regions[4].begin != 512)
            return fail("the header's regions are not the kernel's", T, -1);
        // the tile's reads end inside ring + mirror (a frame that starts in the ring's last chunk runs into the mirror)
        if (hopk::kRingFloats - 4 + hopk::kWindow > (hopk::kRing + 1) * hopk::kChunk) return fail("a frame's reads pass the mirror", T, -1);
        std::set<int> seen;
        for (int w = 0; w < pairp::kWaves; w++) {
            const int a = pairp::word_address(w, kShare), off = a - w * kShare;
            if (a % 4 != 0) return fail("the word is not 4-byte aligned", T, w);
            if (off < 0 || off + 4 > kShare) return fail("the word leaves its wave's share", T, w);
            if (off != pairp::word_offset(kShare)) return fail("word_address and word_offset disagree", T, w);
            if (!seen.insert(a).second) return fail("two waves share a word", T, w);
            for (const Region &r : regions)
                if (off + 4 > r.begin && off < r.end) {
                    std::printf("(%s) ", r.name);
                    return fail("the word overlaps a region", T, w);
                }
        }
        if ((int)seen.size() != pairp::kWaves) return fail("not eight words", T, -1);
    }
    std::printf("ok\n");
    return 0;
}
