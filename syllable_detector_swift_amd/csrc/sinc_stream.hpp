// sinc_stream.hpp -- the index arithmetic of the streaming band-limited resampler (the streaming sinc convention of
// include/syldet.h), in plain C++ for the host, the kernels (kernels_sinc.hip) and the CPU walk (tests/cpp/sinc_stream_walk_test.cpp):
//   N  input samples received so far (a channel), M outputs emitted so far, L = ceil(2 H) + 2 the history's capacity
//   ready     output i is complete once floor(p_i + H) <= N - 1, p_i = (double)i * rate_in / rate_out -- the kernel's own operations
//             in the kernel's own order; ready(N) counts such outputs
//   history   after N samples the handle keeps the last min(N, L) of them, samples [N - min(N, L), N), sample k at offset
//             k - (N - min(N, L)) of the channel's history row
//   locate    during a push of n samples, sample k < N is in the history (at that offset), sample N <= k < N + n is element
//             k - N of the pushed row
//   carry     element j of the next history, j < min(N + n, L), is sample N + n - min(N + n, L) + j, located as above
//   stage     the inputs a workgroup with outputs [i_first, i_last] stages: [max(floor(p_first - H), 0, N - min(N, L)),
//             min(ceil(p_last + H), n_end - 1)], n_end = N + n for a push and N for a flush
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define SD_SINC_HD __host__ __device__
#else
#define SD_SINC_HD
#endif

namespace sd {

// the history's capacity in samples a channel: the next output's first tap is never further behind N (see sinc_stream_first_needed)
inline int64_t sinc_stream_history(double H) { return (int64_t)std::ceil(2.0 * H) + 2; }

SD_SINC_HD inline int64_t sinc_stream_hist_len(int64_t N, int64_t L) { return N < L ? N : L; }
// the first sample the history still holds
SD_SINC_HD inline int64_t sinc_stream_hist_first(int64_t N, int64_t L) { return N - sinc_stream_hist_len(N, L); }
SD_SINC_HD inline bool sinc_stream_in_history(int64_t k, int64_t N) { return k < N; }
SD_SINC_HD inline int64_t sinc_stream_hist_offset(int64_t k, int64_t N, int64_t L) { return k - sinc_stream_hist_first(N, L); }
SD_SINC_HD inline int64_t sinc_stream_push_offset(int64_t k, int64_t N) { return k - N; }
// the sample that element j of the history after a push of n samples holds
SD_SINC_HD inline int64_t sinc_stream_carry_sample(int64_t j, int64_t N, int64_t n, int64_t L) { return sinc_stream_hist_first(N + n, L) + j; }

SD_SINC_HD inline double sinc_stream_position(int64_t i, double rate_in, double rate_out) { return (double)i * rate_in / rate_out; }
SD_SINC_HD inline bool sinc_stream_is_ready(int64_t i, int64_t N, double rate_in, double rate_out, double H)
{
    return (int64_t)::floor(sinc_stream_position(i, rate_in, rate_out) + H) <= N - 1;
}
// the first input output i reads: max(ceil(p_i - H), 0)
SD_SINC_HD inline int64_t sinc_stream_first_needed(int64_t i, double rate_in, double rate_out, double H)
{
    const int64_t k = (int64_t)::ceil(sinc_stream_position(i, rate_in, rate_out) - H);
    return k > 0 ? k : 0;
}
// the stretch of inputs a workgroup stages (empty when hi < lo)
SD_SINC_HD inline int64_t sinc_stream_stage_lo(int64_t i_first, int64_t N, int64_t L, double rate_in, double rate_out, double H)
{
    int64_t lo = (int64_t)::floor(sinc_stream_position(i_first, rate_in, rate_out) - H);
    if (lo < 0) lo = 0;
    const int64_t first = sinc_stream_hist_first(N, L);
    return lo < first ? first : lo;
}
SD_SINC_HD inline int64_t sinc_stream_stage_hi(int64_t i_last, int64_t n_end, double rate_in, double rate_out, double H)
{
    const int64_t hi = (int64_t)::ceil(sinc_stream_position(i_last, rate_in, rate_out) + H);
    return hi < n_end - 1 ? hi : n_end - 1;
}

// ready(N): the number of outputs i >= 0 with sinc_stream_is_ready(i, N).  The predicate is monotone in i (p_i does not decrease), so
// this is the first i that fails it: bracketed around (N - H) * rate_out / rate_in, then bisected.  H >= 4 (Z >= 4, s <= 1).
inline int64_t sinc_stream_ready(int64_t N, double rate_in, double rate_out, double H)
{
    if (N <= 0) return 0;
    int64_t lo = 0;                                                      // every i < lo is ready
    int64_t hi = (int64_t)((double)N * rate_out / rate_in) + 2;          // p_hi + H > N + 2: not ready
    const double est_f = std::floor(((double)N - H) * rate_out / rate_in);
    if (est_f >= 2.0 && est_f < 9.0e18) {
        const int64_t est = (int64_t)est_f;
        if (est - 2 < hi && sinc_stream_is_ready(est - 2, N, rate_in, rate_out, H)) lo = est - 1;
        if (est + 2 < hi && !sinc_stream_is_ready(est + 2, N, rate_in, rate_out, H)) hi = est + 2;
    }
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (sinc_stream_is_ready(mid, N, rate_in, rate_out, H)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace sd
