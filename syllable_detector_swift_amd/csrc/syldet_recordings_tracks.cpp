// syldet_recordings_tracks.cpp -- packed recordings: every recording's output track and trigger track (include/syldet.h, "packed
// recordings: the per-sample tracks"; kernels_recordings_tracks.hip).  The handle (syldet_recordings.hpp) keeps the destination
// layout and the last_seen prefix on the device, beside the plan's tables, so that a call with the kept layout is launches only.

#include "syldet_recordings.hpp"

namespace {

// the destinations: statuses before any device is touched (NULL step: all 1)
int layout_args(const syldet_recordings_t *r, const void *d_dst, int64_t dst_elements, const int64_t *dst_offset, const int32_t *dst_step)
{
    if (dst_elements < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "dst_elements is negative");
    if (r->plan.K > 0 && !dst_offset) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int k = 0; k < r->plan.K; k++) {
        const int64_t step = dst_step ? dst_step[k] : 1, n = r->plan.slots[(size_t)k].n_samples;
        if (dst_offset[k] < 0 || step < 1)
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "a negative destination offset or a step below 1 (recording " + std::to_string(k) + ")");
        // offset + (n - 1) step < dst_elements, without overflow
        if (n > 0 && (dst_offset[k] >= dst_elements || (dst_elements - 1 - dst_offset[k]) / step < n - 1))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "recording " + std::to_string(k) + " of " + std::to_string(n) + " samples at offset " +
                                                         std::to_string(dst_offset[k]) + ", step " + std::to_string(step) + " ends behind the " +
                                                         std::to_string(dst_elements) + " elements of the destination");
        if (n > 0 && !d_dst) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    }
    return SYLDET_OK;
}

int trigger_limits(int32_t L, int64_t N, int64_t latency)
{
    if (int st = buffer_length_arg(L)) return st;
    if (N < 1 || N > ((int64_t)1 << 24)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "width_samples must be in [1, 2^24]");
    if (latency < 0 || latency > ((int64_t)1 << 24)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "latency_samples must be in [0, 2^24]");
    return SYLDET_OK;
}

// The kept destination layout: a layout that differs from it (the first always) is uploaded behind the last track call.
int keep_layout(syldet_recordings_t *r, const int64_t *dst_offset, const int32_t *dst_step)
{
    // the key is the table itself: entry i holds the destination of recording order[i]
    KeptTable<RecTrackDev> &t = r->tracks.layout;
    const std::vector<int32_t> &order = r->plan.order;
    auto entry = [&](size_t i) { return RecTrackDev{dst_offset[order[i]], dst_step ? dst_step[order[i]] : 1, order[i]}; };
    bool same = t.kept;
    for (size_t i = 0; i < order.size() && same; i++) same = t.host[i].dst_offset == entry(i).dst_offset && t.host[i].dst_step == entry(i).dst_step;
    if (same || order.empty()) return SYLDET_OK;
    return t.remake([&]() -> int {
        for (size_t i = 0; i < order.size(); i++) t.host[i] = entry(i);
        return SYLDET_OK;
    });
}

// The kept buffer length: recording k's last_seen table has B'_k = trigger_buffers(n_k, L) entries, the tables lie end to end, and
// the prefix of K + 1 entries is uploaded when L changes -- behind the last track call, one that read the layout alone too; the
// tables themselves are scratch the handle keeps and grows.
int keep_buffers(syldet_recordings_t *r, int32_t L)
{
    syldet_recordings::Tracks &t = r->tracks;
    const std::vector<syldet_slot_t> &slots = r->plan.slots;
    const size_t K = slots.size();
    if ((t.ls_begin.kept && t.L == L) || K == 0) return SYLDET_OK;
    int64_t total = 0;
    for (size_t k = 0; k < K; k++) {
        const int64_t Bp = trigger_buffers(slots[k].n_samples, L);
        if (Bp < 0 || total + Bp > 0x7fffffffLL) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 buffers in all recordings");
        total += Bp;
    }
    return t.ls_begin.remake([&]() -> int {
        t.L = L;
        int32_t at = 0;
        for (size_t k = 0; k < K; k++) {
            t.ls_begin.host[k] = at;
            at += (int32_t)trigger_buffers(slots[k].n_samples, L);
        }
        t.ls_begin.host[K] = at;
        return t.last_seen.reserve((size_t)at * sizeof(int));
    }, t.layout.kept);
}

int trace_impl(syldet_recordings_t *r, const float *d_outputs, int32_t output, void *d_dst, bool s16, int64_t dst_elements,
               const int64_t *dst_offset, const int32_t *dst_step, hipStream_t stream)
{
    if (!r || (r->plan.K > 0 && r->plan.row_evals > 0 && !d_outputs)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (output < 0 || output >= r->bank.geom.outputs) return fail(SYLDET_ERR_INVALID_ARGUMENT, "output outside [0, outputs)");
    if (int st = layout_args(r, d_dst, dst_elements, dst_offset, dst_step)) return st;
    if (r->plan.K == 0 || r->plan.row_samples == 0) return SYLDET_OK;
    syldet *h = r->h;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_layout(r, dst_offset, dst_step)) return st;
    const float *thr = nullptr;
    if (int st = trace_thresholds(h, output, &thr)) return st;
    r->tracks.read_on(stream);
    h->prof_begin();
    KernelTimer t(h, stream, "recordings_trace_kernel");
    SYLDET_HIP(launch_recordings_trace(r->tracks.desc, r->bank.channels, d_outputs, r->bank.geom.outputs, output, thr, d_dst, s16, r->bank.geom.first_index,
                                       r->bank.geom.hop, stream));
    return SYLDET_OK;
}

// the scan every trigger call begins with
int trigger_begin(syldet_recordings_t *r, const uint8_t *d_flags, int32_t L, hipStream_t stream)
{
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_buffers(r, L)) return st;
    r->tracks.read_on(stream);
    r->h->prof_begin();
    KernelTimer t(r->h, stream, "recordings_trigger_scan_kernel");
    SYLDET_HIP(launch_recordings_trigger_scan(r->tracks.desc, d_flags, L, r->bank.geom.first_index, r->bank.geom.hop, (int *)r->tracks.last_seen.ptr, stream));
    return SYLDET_OK;
}

int trigger_impl(syldet_recordings_t *r, const uint8_t *d_flags, int32_t L, int64_t N, int64_t latency, void *d_dst, bool s16, int64_t dst_elements,
                 const int64_t *dst_offset, const int32_t *dst_step, hipStream_t stream)
{
    if (!r || (r->plan.K > 0 && r->plan.row_evals > 0 && !d_flags)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = trigger_limits(L, N, latency)) return st;
    if (int st = layout_args(r, d_dst, dst_elements, dst_offset, dst_step)) return st;
    if (r->plan.K == 0 || r->plan.row_samples == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_layout(r, dst_offset, dst_step)) return st;
    if (int st = trigger_begin(r, d_flags, L, stream)) return st;
    KernelTimer t(r->h, stream, "recordings_trigger_kernel");
    SYLDET_HIP(launch_recordings_trigger(r->tracks.desc, r->bank.channels, (const int *)r->tracks.last_seen.ptr, L, N, latency, d_dst, s16, stream));
    return SYLDET_OK;
}

}  // namespace

extern "C" {

int syldet_recordings_trace_device(syldet_recordings_t *r, const float *d_outputs, int32_t output, float *d_dst, int64_t dst_elements,
                                   const int64_t *dst_offset, const int32_t *dst_step, void *hip_stream)
{
    return trace_impl(r, d_outputs, output, d_dst, false, dst_elements, dst_offset, dst_step, (hipStream_t)hip_stream);
}

int syldet_recordings_trace_device_s16(syldet_recordings_t *r, const float *d_outputs, int32_t output, int16_t *d_dst, int64_t dst_elements,
                                       const int64_t *dst_offset, const int32_t *dst_step, void *hip_stream)
{
    return trace_impl(r, d_outputs, output, d_dst, true, dst_elements, dst_offset, dst_step, (hipStream_t)hip_stream);
}

int syldet_recordings_trigger_device(syldet_recordings_t *r, const uint8_t *d_flags, int32_t buffer_length, int64_t width_samples,
                                     int64_t latency_samples, float *d_dst, int64_t dst_elements, const int64_t *dst_offset,
                                     const int32_t *dst_step, void *hip_stream)
{
    return trigger_impl(r, d_flags, buffer_length, width_samples, latency_samples, d_dst, false, dst_elements, dst_offset, dst_step,
                        (hipStream_t)hip_stream);
}

int syldet_recordings_trigger_device_s16(syldet_recordings_t *r, const uint8_t *d_flags, int32_t buffer_length, int64_t width_samples,
                                         int64_t latency_samples, int16_t *d_dst, int64_t dst_elements, const int64_t *dst_offset,
                                         const int32_t *dst_step, void *hip_stream)
{
    return trigger_impl(r, d_flags, buffer_length, width_samples, latency_samples, d_dst, true, dst_elements, dst_offset, dst_step,
                        (hipStream_t)hip_stream);
}

int syldet_recordings_trigger_onsets_device(syldet_recordings_t *r, const uint8_t *d_flags, int32_t buffer_length, int64_t width_samples,
                                            int64_t latency_samples, int64_t *d_indices, int64_t capacity, int64_t *d_counts, void *hip_stream)
{
    if (!r || (r->plan.K > 0 && r->plan.row_evals > 0 && !d_flags) || (r->plan.K > 0 && !d_counts) || capacity < 0 ||
        (r->plan.K > 0 && capacity > 0 && !d_indices))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (int st = trigger_limits(buffer_length, width_samples, latency_samples)) return st;
    if (r->plan.K == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = trigger_begin(r, d_flags, buffer_length, stream)) return st;
    KernelTimer t(r->h, stream, "recordings_trigger_onsets_kernel");
    SYLDET_HIP(launch_recordings_trigger_onsets(r->tracks.desc, (const int *)r->tracks.last_seen.ptr, buffer_length, width_samples, latency_samples, d_indices,
                                                capacity, d_counts, stream));
    return SYLDET_OK;
}

}  // extern "C"
