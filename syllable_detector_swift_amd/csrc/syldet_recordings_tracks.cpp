// syldet_recordings_tracks.cpp -- packed recordings: every recording's output track and trigger track (include/syldet.h, "packed
// recordings: the per-sample tracks"; kernels_recordings_tracks.hip).  The handle (syldet_recordings.hpp) keeps the destination
// layout and the last_seen prefix on the device, beside the plan's tables, so that a call with the kept layout is launches only.

#include "syldet_handle.hpp"
#include "syldet_recordings.hpp"

namespace {

// the destinations: statuses before any device is touched (NULL step: all 1)
int layout_args(const syldet_recordings_t *r, const void *d_dst, int64_t dst_elements, const int64_t *dst_offset, const int32_t *dst_step)
{
    if (dst_elements < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "dst_elements is negative");
    if (r->K > 0 && !dst_offset) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    for (int k = 0; k < r->K; k++) {
        const int64_t step = dst_step ? dst_step[k] : 1, n = r->slots[(size_t)k].n_samples;
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
    if (!levels_buffer_ok(L)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "buffer_length must be a power of two in [8, 4096]");
    if (N < 1 || N > ((int64_t)1 << 24)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "width_samples must be in [1, 2^24]");
    if (latency < 0 || latency > ((int64_t)1 << 24)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "latency_samples must be in [0, 2^24]");
    return SYLDET_OK;
}

// The kept destination layout: a layout that differs from it (the first always) waits for the stream of the last track call, which
// may still read the table, and uploads once with a blocking copy.
int keep_layout(syldet_recordings_t *r, const int64_t *dst_offset, const int32_t *dst_step)
{
    const int K = r->K;
    bool same = r->track_kept;
    for (int k = 0; k < K && same; k++)
        same = r->track_offset[(size_t)k] == dst_offset[k] && r->track_step[(size_t)k] == (dst_step ? dst_step[k] : 1);
    if (same || K == 0) return SYLDET_OK;
    if (r->track_kept) SYLDET_HIP(hipStreamSynchronize(r->track_last));
    r->track_kept = false;
    r->track_offset.assign(dst_offset, dst_offset + K);      // (reserved by syldet_recordings_create: no allocation)
    r->track_step.assign((size_t)K, 1);
    if (dst_step) r->track_step.assign(dst_step, dst_step + K);
    for (size_t i = 0; i < r->table.size(); i++) {
        const int32_t k = r->order[i];
        r->track_host[i] = sd::RecTrackDev{r->track_offset[(size_t)k], r->track_step[(size_t)k], k};
    }
    hipError_t e = hipMemcpy(r->d_track, r->track_host.data(), r->track_host.size() * sizeof(sd::RecTrackDev), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    r->track_kept = true;
    return SYLDET_OK;
}

// The kept buffer length: recording k's last_seen table has B'_k = trigger_buffers(n_k, L) entries, the tables lie end to end, and
// the prefix of K + 1 entries is uploaded when L changes; the tables themselves are scratch the handle keeps and grows.
int keep_buffers(syldet_recordings_t *r, int32_t L)
{
    const int K = r->K;
    if (r->track_L == L || K == 0) return SYLDET_OK;
    int64_t total = 0;
    for (int k = 0; k < K; k++) {
        const int64_t Bp = trigger_buffers(r->slots[(size_t)k].n_samples, L);
        if (Bp < 0 || total + Bp > 0x7fffffffLL) return fail(SYLDET_ERR_UNSUPPORTED, "more than 2^31 buffers in all recordings");
        total += Bp;
    }
    if (r->track_L != 0 || r->track_kept) SYLDET_HIP(hipStreamSynchronize(r->track_last));
    r->track_L = 0;
    total = 0;
    for (int k = 0; k < K; k++) {
        r->ls_host[(size_t)k] = (int32_t)total;
        total += trigger_buffers(r->slots[(size_t)k].n_samples, L);
    }
    r->ls_host[(size_t)K] = (int32_t)total;
    const size_t bytes = (size_t)total * sizeof(int);
    if (bytes > r->last_seen_cap) {
        if (r->d_last_seen) (void)hipFree(r->d_last_seen);
        r->d_last_seen = nullptr;
        r->last_seen_cap = 0;
        hipError_t e = hipMalloc(&r->d_last_seen, bytes);
        if (e != hipSuccess) {
            r->d_last_seen = nullptr;
            return fail(e == hipErrorOutOfMemory ? SYLDET_ERR_OUT_OF_MEMORY : SYLDET_ERR_DEVICE, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        r->last_seen_cap = bytes;
    }
    hipError_t e = hipMemcpy(r->d_ls_begin, r->ls_host.data(), r->ls_host.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    r->track_L = L;
    return SYLDET_OK;
}

int trace_impl(syldet_recordings_t *r, const float *d_outputs, int32_t output, void *d_dst, bool s16, int64_t dst_elements,
               const int64_t *dst_offset, const int32_t *dst_step, hipStream_t stream)
{
    if (!r || (r->K > 0 && r->row_evals > 0 && !d_outputs)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (output < 0 || output >= r->bank.geom.outputs) return fail(SYLDET_ERR_INVALID_ARGUMENT, "output outside [0, outputs)");
    if (int st = layout_args(r, d_dst, dst_elements, dst_offset, dst_step)) return st;
    if (r->K == 0 || r->row_samples == 0) return SYLDET_OK;
    syldet *h = r->h;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_layout(r, dst_offset, dst_step)) return st;
    const float *thr = nullptr;
    if (int st = trace_thresholds(h, output, &thr)) return st;
    r->track_last = stream;
    h->prof_begin();
    KernelTimer t(h, stream, "recordings_trace_kernel");
    SYLDET_HIP(launch_recordings_trace(r->track, r->bank.channels, d_outputs, r->bank.geom.outputs, output, thr, d_dst, s16, r->bank.geom.first_index,
                                       r->bank.geom.hop, stream));
    return SYLDET_OK;
}

// the scan every trigger call begins with
int trigger_begin(syldet_recordings_t *r, const uint8_t *d_flags, int32_t L, hipStream_t stream)
{
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_buffers(r, L)) return st;
    r->track_last = stream;
    r->h->prof_begin();
    KernelTimer t(r->h, stream, "recordings_trigger_scan_kernel");
    SYLDET_HIP(launch_recordings_trigger_scan(r->track, d_flags, L, r->bank.geom.first_index, r->bank.geom.hop, (int *)r->d_last_seen, stream));
    return SYLDET_OK;
}

int trigger_impl(syldet_recordings_t *r, const uint8_t *d_flags, int32_t L, int64_t N, int64_t latency, void *d_dst, bool s16, int64_t dst_elements,
                 const int64_t *dst_offset, const int32_t *dst_step, hipStream_t stream)
{
    if (!r || (r->K > 0 && r->row_evals > 0 && !d_flags)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = trigger_limits(L, N, latency)) return st;
    if (int st = layout_args(r, d_dst, dst_elements, dst_offset, dst_step)) return st;
    if (r->K == 0 || r->row_samples == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_layout(r, dst_offset, dst_step)) return st;
    if (int st = trigger_begin(r, d_flags, L, stream)) return st;
    KernelTimer t(r->h, stream, "recordings_trigger_kernel");
    SYLDET_HIP(launch_recordings_trigger(r->track, r->bank.channels, (const int *)r->d_last_seen, L, N, latency, d_dst, s16, stream));
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
    if (!r || (r->K > 0 && r->row_evals > 0 && !d_flags) || (r->K > 0 && !d_counts) || capacity < 0 || (r->K > 0 && capacity > 0 && !d_indices))
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (int st = trigger_limits(buffer_length, width_samples, latency_samples)) return st;
    if (r->K == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = trigger_begin(r, d_flags, buffer_length, stream)) return st;
    KernelTimer t(r->h, stream, "recordings_trigger_onsets_kernel");
    SYLDET_HIP(launch_recordings_trigger_onsets(r->track, (const int *)r->d_last_seen, buffer_length, width_samples, latency_samples, d_indices,
                                                capacity, d_counts, stream));
    return SYLDET_OK;
}

}  // extern "C"
