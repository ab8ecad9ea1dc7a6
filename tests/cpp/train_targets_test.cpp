// train_targets_test.cpp -- csrc/train_targets.hpp on the host, alone (no HIP, no library): built with -fsanitize=address,undefined
// by tests/test_train_host.py and run as a program of its own.  It walks train_target_mask and train_target_write over the grid the
// Python tests use -- two clocks (hop 132 and 131), several detector lengths, labels that overlap, repeat, lie before 0 and behind
// the end, half widths 0, 1, hop and 5 hop, one to four outputs -- and checks
//   1. the mask against a walk over every label (no search)
//   2. the floats and the weight against the mask
// with the labels, their outputs and the results in heap blocks of exactly their sizes: a read or a write outside them is an
// AddressSanitizer report, an overflow in the arithmetic a UBSan report.  Prints "ok".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "train_targets.hpp"

namespace {

int failures = 0;

void expect(bool ok, const char *what, long long a = 0, long long b = 0, long long c = 0)
{
    if (ok) return;
    if (failures++ < 20) std::fprintf(stderr, "FAILED: %s (%lld, %lld, %lld)\n", what, a, b, c);
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rng()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

}  // namespace

int main()
{
    const int64_t hops[] = {132, 131};
    const int64_t evals[] = {0, 1, 2, 77, 300};
    long long checked = 0, positives = 0, negatives = 0, several = 0;
    for (int64_t hop : hops) {
        const int64_t first_index = 9 * hop + 256;
        for (int64_t E : evals) {
            const int64_t end = first_index + E * hop;
            for (int n_out = 1; n_out <= sd::kTrainMaxOut; n_out++) {
                for (int n_labels : {0, 1, 2, 7, 40}) {
                    // sorted labels: before 0, behind the end, some repeated, some closer than a hop
                    std::vector<int64_t> sorted;
                    for (int j = 0; j < n_labels; j++) sorted.push_back((int64_t)(rng() % (uint64_t)(end + 4001)) - 2000);
                    if (n_labels >= 2) sorted[1] = sorted[0];
                    if (n_labels >= 7) sorted[6] = sorted[5] + 3;
                    std::sort(sorted.begin(), sorted.end());
                    int64_t *labels = (int64_t *)std::malloc((size_t)(n_labels > 0 ? n_labels : 1) * sizeof(int64_t));
                    int32_t *outs = (int32_t *)std::malloc((size_t)(n_labels > 0 ? n_labels : 1) * sizeof(int32_t));
                    for (int j = 0; j < n_labels; j++) {
                        labels[j] = sorted[(size_t)j];
                        outs[j] = (int32_t)(rng() % (uint64_t)n_out);
                    }
                    float *target = (float *)std::malloc((size_t)n_out * sizeof(float));
                    float *weight = (float *)std::malloc(sizeof(float));
                    for (int64_t hw : {(int64_t)0, (int64_t)1, hop, 5 * hop, sd::kTrainMaxHalfWidth}) {
                        for (int with_outs = 0; with_outs < 2; with_outs++) {
                            for (int64_t e = 0; e < E; e++) {
                                const int64_t idx = first_index + e * hop;
                                uint32_t want = 0;
                                for (int j = 0; j < n_labels; j++) {
                                    const int64_t dist = idx > labels[j] ? idx - labels[j] : labels[j] - idx;
                                    if (dist <= hw) want |= 1u << (with_outs ? outs[j] : 0);
                                }
                                const uint32_t got = sd::train_target_mask(idx, labels, with_outs ? outs : nullptr, n_labels, hw);
                                expect(got == want, "a mask", idx, got, want);
                                sd::train_target_write(got, n_out, 0.25f, 0.125f, target, weight);
                                for (int o = 0; o < n_out; o++) expect(target[o] == ((want >> o) & 1u ? 1.0f : 0.0f), "a target", idx, o);
                                expect(*weight == (want ? 0.25f : 0.125f), "a weight", idx);
                                checked++;
                                (want ? positives : negatives)++;
                                if (want & (want - 1)) several++;
                            }
                        }
                    }
                    std::free(labels);
                    std::free(outs);
                    std::free(target);
                    std::free(weight);
                }
            }
        }
    }
    // the extremes of the sample numbers: |idx| < 2^62 with the widest half width does not overflow
    const int64_t far[] = {sd::kTrainIndexLimit - 1, -(sd::kTrainIndexLimit - 1)};
    const int64_t ends[] = {INT64_MIN, INT64_MAX};
    for (int64_t idx : far) expect(sd::train_target_mask(idx, ends, nullptr, 2, sd::kTrainMaxHalfWidth) == 0, "a mask at the limit", idx);
    expect(positives > 0 && negatives > 0 && several > 0, "a state the grid never reaches", positives, negatives, several);
    if (failures) {
        std::fprintf(stderr, "%d failures in %lld evaluations\n", failures, checked);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
