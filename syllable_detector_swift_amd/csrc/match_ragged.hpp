// match_ragged.hpp -- template matching, a ragged bank (include/syldet.h, "template matching: a ragged bank"): templates of their
// own lengths n_k, lined up at their anchors a_k.  The plan of a tile and the rule of a window, one text for the kernels
// (kernels_match.hip), the host (syldet_match.cpp) and a stand-alone test (tests/cpp/match_ragged_test.cpp).  Integers only.
//   match_tile_floats      the floats of a tile's LDS: G staged frames, one template region of n frames, the frames' energies, the
//                          four waves' sums (match_plan counts a single template's tile with it: G = 255 + n)
//   match_ragged_plan      the lead a_max = max a_k, the tail r_max = max (n_k - a_k), G = 255 + a_max + r_max staged frames (the
//                          frames p0 - a_max .. p0 + 255 + r_max - 1 of a tile whose plane elements are p0 .. p0 + 255), the one
//                          template region of n_max frames, and the form: matrix iff the tile fits 64 KB
//   match_ragged_first     s_k = a_max - a_k: the staged frame at which plane element p0's window of template k begins
//   match_ragged_last      the furthest staged frame a pass of template k's products, or its energy sums, read: 254 + s_k + n_k
//   match_ragged_window    does template k's window at plane element u, the frames [u - a_k, u - a_k + n_k), lie in the detector's
//                          own frames [first, end) -- on BOTH sides
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_MATCH_RAGGED_FN __host__ __device__ __forceinline__
#else
#define SD_MATCH_RAGGED_FN inline
#endif

namespace sd {

constexpr int kMatchTileElements = 256;                      // plane elements (positions) a workgroup of the score kernels takes
constexpr int kMatchLdsBytes = 64 * 1024;                    // the bound of the matrix form's tile

// Fp: floats a staged frame (bins padded to 4); FT: floats a staged template frame (4 x an odd number)
SD_MATCH_RAGGED_FN int64_t match_tile_floats(int64_t G, int64_t n_region, int bins, int *Fp_out, int *FT_out)
{
    const int Fp = (bins + 3) / 4 * 4;
    const int FT = ((Fp / 4) & 1) ? Fp : Fp + 4;
    if (Fp_out) *Fp_out = Fp;
    if (FT_out) *FT_out = FT;
    return G * Fp + 4 * ((G + 15) / 16) + n_region * FT + G + 4 * kMatchTileElements;
}

struct MatchRaggedPlan {
    int a_max, r_max, n_max;
    int G;                                                   // staged frames
    int Fp, FT;
    int64_t floats;
    int matrix, lds_bytes;
};

// n [K], a [K]: 1 <= n_k, 0 <= a_k < n_k (the caller's to check); K >= 1
SD_MATCH_RAGGED_FN MatchRaggedPlan match_ragged_plan(const int32_t *n, const int32_t *a, int K, int bins)
{
    MatchRaggedPlan p{};
    for (int k = 0; k < K; k++) {
        if (a[k] > p.a_max) p.a_max = a[k];
        if (n[k] - a[k] > p.r_max) p.r_max = n[k] - a[k];
        if (n[k] > p.n_max) p.n_max = n[k];
    }
    p.G = kMatchTileElements - 1 + p.a_max + p.r_max;
    p.floats = match_tile_floats(p.G, p.n_max, bins, &p.Fp, &p.FT);
    p.matrix = p.floats * 4 <= kMatchLdsBytes;
    p.lds_bytes = p.matrix ? (int)(p.floats * 4) : 0;
    return p;
}

SD_MATCH_RAGGED_FN int match_ragged_first(const MatchRaggedPlan &p, int a_k) { return p.a_max - a_k; }

// row 15 of the A operand reads the frames 240 + s_k + f, f < n_k + 15; plane element 255 sums the energies 255 + s_k + j, j < n_k
SD_MATCH_RAGGED_FN int match_ragged_last(const MatchRaggedPlan &p, int n_k, int a_k)
{
    return kMatchTileElements - 2 + match_ragged_first(p, a_k) + n_k;
}

SD_MATCH_RAGGED_FN bool match_ragged_window(int64_t first, int64_t end, int64_t u, int a_k, int n_k)
{
    return u - a_k >= first && u - a_k + n_k <= end;
}

}  // namespace sd
