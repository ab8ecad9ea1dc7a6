// detections_scan.hpp -- the debounce scan of TrackDetector.swift:39-43, :65-100 as one wave runs it: 64 flags a step, ballots,
// one load per 64 evaluations over quiet stretches.  Shared by detections_kernel (kernels_generic.hip: one wave a channel) and
// recordings_events_kernel (kernels_recordings.hip: one wave a recording of a packed row).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace sd {

// fl [E]: the flags of one detector from its first evaluation on.  emit(n, e, idx) is called by the whole wave (uniform
// arguments) for detection n, in order: evaluation e, sample number idx = first_index + e hop.  Returns how many there are.
template <class Emit>
__device__ __forceinline__ int64_t debounce_scan(const uint8_t *__restrict__ fl, int64_t E, int64_t first_index, int64_t hop,
                                                 int64_t debounce_frames, int lane, Emit emit)
{
    int64_t until = -1;      // debounceUntil :30
    int64_t n = 0;
    for (int64_t e0 = 0; e0 < E; e0 += 64) {
        const int64_t e = e0 + lane;
        const bool set = e < E && fl[e] != 0;
        const int64_t idx = first_index + e * hop;               // curOutput :67-68
        unsigned long long mask = __ballot(set && until < idx);  // hasDetection && debounceUntil < curOutput :80
        while (mask) {
            const int l = __ffsll((long long)mask) - 1;
            const int64_t hit = first_index + (e0 + l) * hop;
            emit(n, e0 + l, hit);
            n++;
            until = hit + debounce_frames;                       // :99
            const unsigned long long later = (l == 63) ? 0ull : (~0ull << (l + 1));
            mask = __ballot(set && until < idx) & later;
        }
    }
    return n;
}

}  // namespace sd
