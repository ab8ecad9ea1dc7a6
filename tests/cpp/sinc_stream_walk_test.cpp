// sinc_stream_walk_test.cpp -- walks csrc/sinc_stream.hpp on the CPU, the way the streaming kernels of kernels_sinc.hip use it, with
// the sample's own index standing for its value.  For seven ratios, four qualities and random partitions (pushes of 0, of 1, of
// the callback's 32, shorter than the filter, longer than a workgroup's stage), started at N = 0 and in the middle of a stream
// near 2^24 and 2^40, after every push:
//   - M = ready(N), ready is monotone, ready(N) <= count(N), and ready(N) is exactly the first output that fails the predicate;
//   - the next output's first tap is no further behind N than the history holds (ceil(2 H) + 2);
//   - every index a workgroup's staging loop reads lies inside the buffer it names (history row of L floats, pushed row of n),
//     and it reads the sample it meant to; every tap of every emitted output lies inside its workgroup's staged stretch;
//   - the carry writes inside the other history row, and that row then holds the last min(N, L) samples of a plain
//     concatenation.
// Prints "ok" and exits 0; the first failure prints its case and exits 1.  Built plain and with -fsanitize=address,undefined.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sinc_stream.hpp"

namespace {

constexpr int kBlockOut = 1024;      // kSincBlockOut
constexpr int kStage = 4000;         // kSincStage

struct Case { double ri, ro; int Z; double rho; };

#define REQUIRE(cond)                                                                                                           \
    do {                                                                                                                        \
        if (!(cond)) {                                                                                                          \
            std::printf("FAILED %s (line %d): %g -> %g, Z %d, start %lld, N %lld, push %lld\n", #cond, __LINE__, c.ri, c.ro, c.Z, \
                        (long long)start, (long long)N, (long long)n);                                                          \
            return false;                                                                                                       \
        }                                                                                                                       \
    } while (0)

int64_t count_outputs(int64_t n_in, double ri, double ro)        // syldet_convert_rate_count
{
    return n_in <= 0 ? 0 : (int64_t)((double)(n_in - 1) * ro / ri) + 1;
}

// One stream: starts with `start` samples already received (history filled as the pushes before would have left it), then
// `pushes`, then a flush.  Samples are their own indices (as doubles: exact below 2^53).
bool walk(const Case &c, int64_t start, const std::vector<int64_t> &pushes)
{
    const double s = std::min(1.0, c.ro / c.ri) * c.rho, H = (double)c.Z / s;
    const int64_t L = sd::sinc_stream_history(H);
    int64_t N = start, n = 0;
    int64_t M = sd::sinc_stream_ready(N, c.ri, c.ro, H);
    std::vector<double> hist[2] = {std::vector<double>((size_t)L, -1.0), std::vector<double>((size_t)L, -1.0)};
    int cur = 0;
    for (int64_t j = 0; j < sd::sinc_stream_hist_len(N, L); j++) hist[cur][(size_t)j] = (double)(sd::sinc_stream_hist_first(N, L) + j);

    auto emit = [&](int64_t n_push, int64_t n_end, int64_t n_emit) -> bool {
        n = n_push;
        for (int64_t i0 = M; i0 < M + n_emit; i0 += kBlockOut) {
            const int64_t i_last = std::min(i0 + kBlockOut, M + n_emit) - 1;
            const int64_t lo = sd::sinc_stream_stage_lo(i0, N, L, c.ri, c.ro, H), hi = sd::sinc_stream_stage_hi(i_last, n_end, c.ri, c.ro, H);
            REQUIRE(lo >= 0 && hi <= n_end - 1);
            for (int64_t base = lo; base <= hi; base += kStage) {
                const int64_t end = std::min(base + kStage - 1, hi);
                for (int64_t k = base; k <= end; k++) {
                    if (sd::sinc_stream_in_history(k, N)) {
                        const int64_t o = sd::sinc_stream_hist_offset(k, N, L);
                        REQUIRE(o >= 0 && o < sd::sinc_stream_hist_len(N, L) && o < L);
                        REQUIRE(hist[cur][(size_t)o] == (double)k);
                    } else {
                        const int64_t o = sd::sinc_stream_push_offset(k, N);
                        REQUIRE(o >= 0 && o < n_push);                   // (the pushed row's element o is sample N + o)
                    }
                }
            }
            // every tap of the first and the last output of the workgroup (the extremes: positions grow with i) is staged
            for (int64_t i : {i0, i_last}) {
                const double p = sd::sinc_stream_position(i, c.ri, c.ro);
                const int64_t k_lo = std::max((int64_t)std::ceil(p - H), (int64_t)0), k_hi = std::min((int64_t)std::floor(p + H), n_end - 1);
                REQUIRE(k_lo == sd::sinc_stream_first_needed(i, c.ri, c.ro, H));
                REQUIRE(k_lo > k_hi || (k_lo >= lo && k_hi <= hi));
                if (n_end > N) REQUIRE((int64_t)std::floor(p + H) <= n_end - 1);      // a push emits complete outputs only
            }
        }
        return true;
    };

    for (int64_t n_push : pushes) {
        n = n_push;
        const int64_t before = sd::sinc_stream_ready(N, c.ri, c.ro, H);
        REQUIRE(before == M);
        const int64_t after = sd::sinc_stream_ready(N + n_push, c.ri, c.ro, H);
        REQUIRE(after >= before && after <= count_outputs(N + n_push, c.ri, c.ro));
        REQUIRE(after == 0 || sd::sinc_stream_is_ready(after - 1, N + n_push, c.ri, c.ro, H));
        REQUIRE(!sd::sinc_stream_is_ready(after, N + n_push, c.ri, c.ro, H));
        // the history bound: the next output's first tap is within L of N
        REQUIRE(N - sd::sinc_stream_first_needed(M, c.ri, c.ro, H) <= L);
        REQUIRE(sd::sinc_stream_first_needed(M, c.ri, c.ro, H) >= sd::sinc_stream_hist_first(N, L));
        if (n_push == 0) continue;
        if (!emit(n_push, N + n_push, after - M)) return false;
        // the carry, into the other buffer
        std::vector<double> &next = hist[cur ^ 1];
        const int64_t len = sd::sinc_stream_hist_len(N + n_push, L);
        REQUIRE(len <= L);
        for (int64_t j = 0; j < len; j++) {
            const int64_t k = sd::sinc_stream_carry_sample(j, N, n_push, L);
            double v;
            if (sd::sinc_stream_in_history(k, N)) {
                const int64_t o = sd::sinc_stream_hist_offset(k, N, L);
                REQUIRE(o >= 0 && o < sd::sinc_stream_hist_len(N, L));
                v = hist[cur][(size_t)o];
            } else {
                const int64_t o = sd::sinc_stream_push_offset(k, N);
                REQUIRE(o >= 0 && o < n_push);
                v = (double)(N + o);
            }
            next[(size_t)j] = v;
        }
        N += n_push;
        M = after;
        cur ^= 1;
        // ... equals the last min(N, L) samples of the concatenation
        for (int64_t j = 0; j < len; j++) REQUIRE(hist[cur][(size_t)j] == (double)(N - len + j));
    }
    // the flush: the row ends at N, no pushed rows
    const int64_t total = count_outputs(N, c.ri, c.ro);
    REQUIRE(total >= M);
    REQUIRE(total == M || sd::sinc_stream_first_needed(M, c.ri, c.ro, H) >= sd::sinc_stream_hist_first(N, L));
    return emit(0, N, total - M);
}

}  // namespace

int main()
{
    const double ratios[7][2] = {{48000.0, 44100.0}, {44100.0, 48000.0}, {96000.0, 44100.0}, {22050.0, 44100.0}, {24414.0625, 44100.0},
                                 {16.0, 1.0}, {1.0, 16.0}};
    const int Zs[4] = {4, 8, 32, 64};
    std::mt19937_64 rng(20241019);
    long walks = 0;
    for (const auto &r : ratios)
        for (int Z : Zs) {
            const Case c{r[0], r[1], Z, Z == 8 ? 0.8 : 0.9};
            const double H = (double)Z / (std::min(1.0, c.ro / c.ri) * c.rho);
            for (int64_t start : {(int64_t)0, ((int64_t)1 << 24) - 40, ((int64_t)1 << 40) + 3}) {
                for (int trial = 0; trial < 6; trial++) {
                    std::vector<int64_t> pushes;
                    int64_t budget = 3000 + (int64_t)(4.0 * H);
                    if (trial == 0) pushes = {0, 1, 1, 7, 64, 0, 500, 1, 1023, 1024, budget};
                    else if (trial == 1) pushes.assign(120, 32);
                    else if (trial == 2) { pushes.assign(300, 1); pushes.push_back(budget); }
                    else if (trial == 3) pushes = {budget + 9000};                       // one push: several stages, several workgroups
                    else
                        while (budget > 0) {
                            const int kind = (int)(rng() % 5);
                            int64_t n = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? (int64_t)(rng() % 100) : kind == 3 ? (int64_t)(rng() % 3000)
                                                                                                                  : (int64_t)(rng() % (uint64_t)(2.5 * H + 2));
                            pushes.push_back(n);
                            budget -= n + 1;
                        }
                    if (!walk(c, start, pushes)) return 1;
                    walks++;
                }
            }
            // ready(N) for every small N against a literal count
            int64_t prev = 0;
            for (int64_t N = 0; N < 3000; N++) {
                int64_t lit = 0;
                while (sd::sinc_stream_is_ready(lit, N, c.ri, c.ro, H)) lit++;
                const int64_t got = sd::sinc_stream_ready(N, c.ri, c.ro, H);
                if (got != lit || got < prev || got > count_outputs(N, c.ri, c.ro)) {
                    std::printf("FAILED ready(%lld) = %lld, literal %lld (%g -> %g, Z %d)\n", (long long)N, (long long)got, (long long)lit, c.ri, c.ro, Z);
                    return 1;
                }
                prev = got;
            }
        }
    if (walks != 7 * 4 * 3 * 6) return 1;
    std::printf("ok\n");
    return 0;
}
