// trigger_pulse.hpp -- the streaming TTL output of one channel: the reference's monostable (AudioInterface.swift), host only.
//   arm     createHighOutput (:442-445): outputHighFor[channel] = width -- set, not added to
//   render  renderOutput (:13-40): high = outputHighFor[channel]; if 0 < high, the counter goes down by min(high, frames);
//           frame i of the buffer is 1.0 for i < high, else 0.0
// The counter is an atomic: the consumer arms while an audio-output thread renders.  An arm that lands between a render's read
// and its write-back is kept (the render's decrement belongs to the pulse it read).
#pragma once

#include <atomic>
#include <cstdint>

namespace sd {

inline void trigger_pulse_arm(std::atomic<int64_t> &high, int64_t width_samples)
{
    high.store(width_samples, std::memory_order_release);
}

inline void trigger_pulse_render(std::atomic<int64_t> &high, float *out, int32_t n_frames)
{
    int64_t h = high.load(std::memory_order_acquire);
    if (0 < h) {
        const int64_t used = h < (int64_t)n_frames ? h : (int64_t)n_frames;
        (void)high.compare_exchange_strong(h, h - used, std::memory_order_acq_rel);   // (h is not used again if it fails: see above)
        h = used;
    }
    for (int32_t i = 0; i < n_frames; i++) out[i] = (int64_t)i < h ? 1.0f : 0.0f;
}

}  // namespace sd
