// levels_values.hpp -- the value arithmetic of the two level meters, shared by the kernels that meter one recording a row
// (kernels_levels.hip) and the kernels that meter the recordings of a packed bank (kernels_recordings_levels.hip): one statement
// of each value, so the two paths cannot drift apart.
//   load_each, group_sum   the 16 bytes a lane holds, and the lowest levels of sum_squares_tree over them
//   xor_add, lanes_sum     the tree's next levels across the lanes of a wave
//   lds_tree               its upper levels, for buffers longer than a wave's reach
//   best_of_lane / _wave   StatMax over a reading's mean squares, written as comparisons
//   levels_out_value       one reading of the output meter
// Every file that includes it is compiled with -ffp-contract=off and without fast-math (see the Makefile): a square, an addition,
// each rounds on its own.
//
// gfx950 only.  wave = 64, workgroups of 256 lanes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sd {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// p + (p of lane ^ D).  Distances 1 and 2 are quad permutations; 4 and 8 are the mirrors of 8 and 16 lanes, which are the xor
// exchanges here because the lanes of a group of D already hold one value; 16 and 32 go through the permute network.
template <int D>
__device__ __forceinline__ float xor_add(float p)
{
    if constexpr (D == 1) return p + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0xB1, 0xf, 0xf, false));
    else if constexpr (D == 2) return p + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x4E, 0xf, 0xf, false));
    else if constexpr (D == 4) return p + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x141, 0xf, 0xf, false));
    else if constexpr (D == 8) return p + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x140, 0xf, 0xf, false));
    else return p + __shfl_xor(p, D);
}

// the 16 bytes of the group at sample s, element by element (rows off a 16-byte line, a row's last partial group): n live samples,
// zeros behind them -- never read
__device__ __forceinline__ u32x4 load_each(const float *row, int64_t s, int n)
{
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; i++)
        if (i < n) v[i] = __float_as_uint(row[s + i]);
    return v;
}
__device__ __forceinline__ u32x4 load_each(const int16_t *row, int64_t s, int n)
{
    u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 8; i++)
        if (i < n) v[i >> 1] |= (unsigned)(uint16_t)row[s + i] << (16 * (i & 1));
    return v;
}

// the tree over a lane's group: (x0^2 + x1^2) + (x2^2 + x3^2), and for eight int16 one level more
template <typename T>
__device__ __forceinline__ float group_sum(u32x4 v)
{
    if constexpr (sizeof(T) == 4) {
        const float a = __uint_as_float(v[0]), b = __uint_as_float(v[1]), c = __uint_as_float(v[2]), d = __uint_as_float(v[3]);
        return (a * a + b * b) + (c * c + d * d);
    } else {
        float q[8];
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float x = (float)(int16_t)(uint16_t)(v[i >> 1] >> (16 * (i & 1))) * (1.0f / 32768.0f);   // exact
            q[i] = x * x;
        }
        return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
    }
}

// a lane's group, then the tree across the lpb lanes of a buffer (lpb a power of two; past 64: the wave's sum).  Lane groups are
// counted from the tree's first leaf, so the xor partners are the tree's siblings.
template <typename T>
__device__ __forceinline__ float lanes_sum(u32x4 raw, int lpb)
{
    float p = group_sum<T>(raw);
    if (lpb > 1) p = xor_add<1>(p);
    if (lpb > 2) p = xor_add<2>(p);
    if (lpb > 4) p = xor_add<4>(p);
    if (lpb > 8) p = xor_add<8>(p);
    if (lpb > 16) p = xor_add<16>(p);
    if (lpb > 32) p = xor_add<32>(p);
    return p;
}

// buffers longer than a wave's reach: r = L / kReach consecutive wave sums each, the tree's upper levels in LDS (sums holds
// kSpan / kReach of them, written and fenced by the caller; returns r, buffer q's sum is then sums[q r])
template <int kSpan, int kReach>
__device__ __forceinline__ int lds_tree(float *sums, int L, int tid)
{
    const int r = L > kReach ? L / kReach : 1;
    for (int d = 1; d < r; d <<= 1) {
        if (tid < kSpan / kReach / (2 * d)) sums[2 * d * tid] += sums[2 * d * tid + d];
        __syncthreads();
    }
    return r;
}

// the greatest of value(b), lo <= b < hi, that is not NaN (-1: none; a mean square is never negative): a lane ...
template <class Value>
__device__ __forceinline__ double best_of_lane(int64_t lo, int64_t hi, Value value)
{
    double best = -1.0;
    for (int64_t b = lo; b < hi; b++) {
        const double v = value(b);
        if (v == v && v > best) best = v;
    }
    return best;
}
// ... or a wave (the greatest of values that are not NaN does not depend on the order); every lane returns it
template <class Value>
__device__ __forceinline__ double best_of_wave(int64_t lo, int64_t hi, int lane, Value value)
{
    double best = -1.0;
    for (int64_t b = lo + lane; b < hi; b += 64) {
        const double v = value(b);
        if (v == v && v > best) best = v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double o = __shfl_xor(best, d);
        if (o > best) best = o;
    }
    return best;
}

// Reading m of a row of n_samples samples and n_evals evaluations, `row` at its evaluation 0 of the metered output: the
// evaluations [ce(min(m P L, S)), ce(min((m + 1) P L, S))), each cut at n_evals, where ce is syldet_count_evals (`need` = gap +
// window).  StatMax: the first value if it is NaN, else the first of the greatest values that are not NaN (a later equal value
// does not replace: -0 in front of +0 stays).  No evaluation: 0.  WAVE: the 64 lanes of a wave share the reading (lane 0 .. 63,
// every lane returns the value), else one lane has it (lane 0).
template <bool WAVE>
__device__ __forceinline__ float levels_out_value(const float *__restrict__ row, int64_t n_evals, int n_out, int64_t m, int64_t n_samples,
                                                  int64_t PL, int64_t need, int64_t hop, int T, int lane)
{
    constexpr int step = WAVE ? 64 : 1;
    auto ce = [&](int64_t s) {
        const int64_t J = s < need ? 0 : (s - need) / hop + 1;
        return min(J >= T ? J - T + 1 : (int64_t)0, n_evals);
    };
    const int64_t e0 = ce(min(m * PL, n_samples)), e1 = ce(min((m + 1) * PL, n_samples));
    float result = 0.0f;
    if (e0 < e1) {
        const float first = row[e0 * n_out];
        float best = 0.0f;
        int64_t at = -1;                               // where `best` is from (-1: no value yet)
        for (int64_t e = e0 + lane; e < e1; e += step) {
            const float v = row[e * n_out];
            if (v == v && (at < 0 || v > best)) { best = v; at = e; }
        }
        if (WAVE) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float ob = __shfl_xor(best, d);
                const long long oa = __shfl_xor((long long)at, d);
                if (oa >= 0 && (at < 0 || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
            }
        }
        result = first != first ? first : best;
    }
    return result;
}

}  // namespace sd
