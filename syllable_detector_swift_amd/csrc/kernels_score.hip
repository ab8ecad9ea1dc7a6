// kernels_score.hip -- threshold calibration (syldet_score_device of include/syldet.h): the debounce scan of
// TrackDetector.swift:65-100 run for K thresholds at once and every emitted detection classed against labelled sample numbers.
//
//   score_kernel   one wave a (detector, group of 64 thresholds); a lane is a threshold.  A step loads 64 evaluations of the one
//                  output, coalesced (the loads of four steps are issued together); where none of them reaches the group's
//                  smallest threshold the wave goes on (one ballot, one uniform branch: a quiet stretch costs a load and a
//                  ballot per 64 evaluations, as in debounce_scan).  Otherwise it
//                  visits, in order, the evaluations that do: the value comes to all lanes by a lane read with a scalar index,
//                  the label cursor moves on scalar registers, and each lane updates its own until, hit bit and six counters
//                  with selects (score_scan.hpp).  No LDS, no atomics, no scratch; a lane's six int64 leave by vector stores.
//
// One detector is one sequential chain (the debounce): a detector is not split along time.  gfx950 only: wave = 64 lanes.

#include "kernels.hpp"
#include "score_scan.hpp"

namespace sd {

namespace {

constexpr int kWave = 64;
constexpr int kLoads = 4;                    // steps of 64 evaluations whose loads are in flight together

__global__ void __launch_bounds__(kWave)
score_kernel(ScoreDesc d, const float *__restrict__ outputs, int64_t n_evals, int n_out, int output, int64_t first_index, int64_t hop,
             int64_t *__restrict__ table)
{
    const int lane = threadIdx.x;
    const int groups = (d.K + kWave - 1) / kWave;
    const int det = __builtin_amdgcn_readfirstlane((int)(blockIdx.x / (unsigned)groups));
    const int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x % (unsigned)groups));
    // the detector's evaluations: a channel's row, or a recording's own part of its row
    int64_t base = (int64_t)det * n_evals, E = n_evals;
    if (d.slots) {
        const DetSpan s = d.slots[det];
        base = (int64_t)s.row * n_evals + s.first;
        E = s.units;
    }
    const int k = g * kWave + lane;
    const float thr = k < d.K ? d.thresholds[k] : __builtin_inff();       // (a lane without a threshold: its row is never written)
    const float least = d.group_least[g];
    const int64_t l0 = d.label_begin[det], n = d.label_begin[det + 1] - l0;
    const int64_t *__restrict__ labels = d.labels + l0;
    const int64_t m = d.tolerance, debounce_frames = d.debounce_frames;
    const float *__restrict__ val = outputs + base * n_out + output;

    ScoreLane s;
    ScoreCursor c = score_cursor_start(labels, n);                        // the label cursor: the wave's, in scalar registers
    for (int64_t e0 = 0; e0 < E; e0 += kWave * kLoads) {
        // kLoads steps' loads are issued together: a quiet stretch waits for memory once per kLoads x 64 evaluations
        float v[kLoads];
#pragma unroll
        for (int u = 0; u < kLoads; u++) {
            const int64_t e = e0 + u * kWave + lane;
            v[u] = e < E ? val[e * n_out] : __builtin_nanf("");           // NaN never fires: neither does the row's end
        }
#pragma unroll
        for (int u = 0; u < kLoads; u++) {
            unsigned long long mask = __ballot(v[u] >= least);
            while (mask) {
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
                mask &= mask - 1;
                const float vl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[u]), l));
                const int64_t idx = first_index + (e0 + u * kWave + l) * hop;   // curOutput :67-68
                score_visit(s, vl >= thr, idx, debounce_frames, labels, n, m, c);
            }
        }
    }
    if (k < d.K) {
        int64_t *row = table + ((int64_t)det * d.K + k) * kScoreColumns;
#pragma unroll
        for (int c = 0; c < kScoreColumns; c++) row[c] = s.n[c];
    }
}

}  // namespace

hipError_t launch_score(const ScoreDesc &d, int D, const float *outputs, int64_t n_evals, int n_out, int output, int64_t first_index,
                        int64_t hop, int64_t *table, hipStream_t stream)
{
    if (D <= 0 || d.K <= 0) return hipSuccess;
    const unsigned groups = (unsigned)((d.K + kWave - 1) / kWave);
    hipLaunchKernelGGL(score_kernel, dim3((unsigned)D * groups), dim3(kWave), 0, stream, d, outputs, n_evals, n_out, output, first_index, hop,
                       table);
    return hipGetLastError();
}

}  // namespace sd
