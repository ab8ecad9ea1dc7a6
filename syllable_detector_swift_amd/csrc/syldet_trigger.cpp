// syldet_trigger.cpp -- the TTL trigger track (Processor.swift:128-148, AudioInterface.swift:13-40, :442-445; kernels_trigger.hip)

#include "syldet_handle.hpp"
#include "trigger_pulse.hpp"

static int trigger_args(const syldet *h, const void *flags, int64_t n_evals, int32_t L, int64_t N, int64_t latency, int64_t n_samples)
{
    if (!h || !flags) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_evals < 0 || n_samples < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "negative size");
    if (int st = buffer_length_arg(L)) return st;
    if (N < 1 || N > ((int64_t)1 << 24)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "width_samples must be in [1, 2^24]");
    if (latency < 0 || latency > ((int64_t)1 << 24)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "latency_samples must be in [0, 2^24]");
    if (trigger_buffers(n_samples, L) < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "n_samples: more than 2^31 buffers");
    return SYLDET_OK;
}

static int trigger_track_args(const syldet *h, const void *flags, int64_t n_evals, int32_t L, int64_t N, int64_t latency, const void *track,
                              int64_t n_samples, int64_t stride)
{
    if (!track) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = trigger_args(h, flags, n_evals, L, N, latency, n_samples)) return st;
    if (stride < n_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "track_stride < n_samples");
    return SYLDET_OK;
}

// the scan: flags -> the handle's last_seen table (every trigger call begins with it)
static int trigger_scan_on_stream(syldet *h, const uint8_t *d_flags, int64_t n_evals, int32_t L, int64_t n_samples, hipStream_t stream)
{
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    if (int st = h->d_trigger_last.reserve((size_t)C * (size_t)trigger_buffers(n_samples, L) * sizeof(int))) return st;
    h->prof_begin();
    KernelTimer t(h, stream, "trigger_scan_kernel");
    SYLDET_HIP(launch_trigger_scan(d_flags, n_evals, C, L, n_samples, h->geom.first_index, h->geom.hop, (int *)h->d_trigger_last.ptr, stream));
    return SYLDET_OK;
}

// T: float or int16_t rows [C][stride]; frames: int16 [n_samples][C] instead, or (d_samples) [n_samples][2 C] with the audio
template <class T>
static int trigger_on_stream(syldet *h, const uint8_t *d_flags, int64_t n_evals, int32_t L, int64_t N, int64_t latency, T *d_track,
                             int64_t n_samples, int64_t stride, bool frames, const int16_t *d_samples, int64_t sample_stride, hipStream_t stream)
{
    if (n_samples == 0) return SYLDET_OK;
    if (int st = trigger_scan_on_stream(h, d_flags, n_evals, L, n_samples, stream)) return st;
    const int C = h->channels;
    const int *last = (const int *)h->d_trigger_last.ptr;
    if constexpr (sizeof(T) == 2) {
        if (frames) {
            KernelTimer t(h, stream, (C == 1 && !d_samples) ? "trigger_kernel" : "trigger_interleaved_s16_kernel");   // (one channel: the planar kernel)
            SYLDET_HIP(launch_trigger_interleaved_s16(last, C, L, N, latency, d_samples, sample_stride, d_track, n_samples, stream));
            return SYLDET_OK;
        }
        KernelTimer t(h, stream, "trigger_kernel");
        SYLDET_HIP(launch_trigger_s16(last, C, L, N, latency, d_track, n_samples, stride, stream));
    } else {
        KernelTimer t(h, stream, "trigger_kernel");
        SYLDET_HIP(launch_trigger(last, C, L, N, latency, d_track, n_samples, stride, stream));
    }
    return SYLDET_OK;
}

// one scan, then the planar track and the onsets
template <class T>
static int trigger_rehearse(syldet *h, const uint8_t *d_flags, int64_t n_evals, int32_t L, int64_t N, int64_t latency, T *d_track, int64_t n_samples,
                            int64_t stride, int64_t *d_indices, int64_t capacity, int64_t *d_counts, hipStream_t stream)
{
    if (!d_counts || capacity < 0 || (capacity > 0 && !d_indices)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (int st = trigger_track_args(h, d_flags, n_evals, L, N, latency, d_track, n_samples, stride)) return st;
    if (int st = trigger_scan_on_stream(h, d_flags, n_evals, L, n_samples, stream)) return st;
    const int *last = (const int *)h->d_trigger_last.ptr;
    if (n_samples > 0) {
        KernelTimer t(h, stream, "trigger_kernel");
        if constexpr (sizeof(T) == 2) SYLDET_HIP(launch_trigger_s16(last, h->channels, L, N, latency, d_track, n_samples, stride, stream));
        else SYLDET_HIP(launch_trigger(last, h->channels, L, N, latency, d_track, n_samples, stride, stream));
    }
    KernelTimer t(h, stream, "trigger_onsets_kernel");
    SYLDET_HIP(launch_trigger_onsets(last, h->channels, L, N, latency, n_samples, d_indices, capacity, d_counts, stream));
    return SYLDET_OK;
}

// the caller's flags on the device (the handle's staging buffer; pump_mu held)
static int trigger_stage_flags(syldet *h, const uint8_t *flags, int64_t n_evals)
{
    const size_t fl_bytes = (size_t)h->channels * (size_t)n_evals;
    if (int st = h->d_stage_flags.reserve(std::max<size_t>(fl_bytes, 1))) return st;
    if (fl_bytes) SYLDET_HIP(hipMemcpyAsync(h->d_stage_flags.ptr, flags, fl_bytes, hipMemcpyHostToDevice, h->stream));
    return SYLDET_OK;
}

template <class T>
static int trigger_host(syldet *h, const uint8_t *flags, int64_t n_evals, int32_t L, int64_t N, int64_t latency, T *track, int64_t n_samples,
                        int64_t stride)
{
    if (int st = trigger_track_args(h, flags, n_evals, L, N, latency, track, n_samples, stride)) return st;
    if (n_samples == 0) return SYLDET_OK;
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    const int64_t ws = (n_samples + 7) & ~(int64_t)7;  // rows of whole 16-byte groups
    if (int st = trigger_stage_flags(h, flags, n_evals)) return st;
    if (int st = h->d_trigger.reserve((size_t)C * (size_t)ws * sizeof(T))) return st;
    if (int st = trigger_on_stream(h, (const uint8_t *)h->d_stage_flags.ptr, n_evals, L, N, latency, (T *)h->d_trigger.ptr, n_samples, ws, false,
                                   nullptr, 0, h->stream))
        return st;
    SYLDET_HIP(hipMemcpy2DAsync(track, (size_t)stride * sizeof(T), h->d_trigger.ptr, (size_t)ws * sizeof(T), (size_t)n_samples * sizeof(T),
                                (size_t)C, hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

extern "C" {

int64_t syldet_trigger_width(double seconds, double rate)
{
    const double x = seconds * rate;                                   // AudioInterface.swift:444
    if (!(x >= 1.0) || !(x < 9.0e18)) return -1;                       // (NaN fails the first comparison)
    return (int64_t)x;
}

int syldet_trigger_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                          int64_t latency_samples, float *d_track, int64_t n_samples, int64_t track_stride, void *hip_stream)
{
    if (int st = trigger_track_args(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_track, n_samples, track_stride)) return st;
    return trigger_on_stream(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_track, n_samples, track_stride, false,
                             nullptr, 0, (hipStream_t)hip_stream);
}

int syldet_trigger_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                              int64_t latency_samples, int16_t *d_track, int64_t n_samples, int64_t track_stride, void *hip_stream)
{
    if (int st = trigger_track_args(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_track, n_samples, track_stride)) return st;
    return trigger_on_stream(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_track, n_samples, track_stride, false,
                             nullptr, 0, (hipStream_t)hip_stream);
}

int syldet_trigger_interleaved_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                          int64_t latency_samples, int16_t *d_frames, int64_t n_samples, void *hip_stream)
{
    if (int st = trigger_track_args(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_frames, n_samples, n_samples)) return st;
    return trigger_on_stream(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_frames, n_samples, n_samples, true, nullptr,
                             0, (hipStream_t)hip_stream);
}

int syldet_trigger_mux_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                  int64_t latency_samples, const int16_t *d_samples, int64_t channel_stride, int16_t *d_frames,
                                  int64_t n_samples, void *hip_stream)
{
    if (!d_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = trigger_track_args(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_frames, n_samples, n_samples)) return st;
    if (channel_stride < n_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride < n_samples");
    return trigger_on_stream(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_frames, n_samples, n_samples, true, d_samples,
                             channel_stride, (hipStream_t)hip_stream);
}

int syldet_trigger_onsets_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                 int64_t latency_samples, int64_t n_samples, int64_t *d_indices, int64_t capacity, int64_t *d_counts,
                                 void *hip_stream)
{
    if (!d_counts || capacity < 0 || (capacity > 0 && !d_indices)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (int st = trigger_args(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, n_samples)) return st;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = trigger_scan_on_stream(h, d_flags, n_evals, buffer_length, n_samples, stream)) return st;
    KernelTimer t(h, stream, "trigger_onsets_kernel");
    SYLDET_HIP(launch_trigger_onsets((const int *)h->d_trigger_last.ptr, h->channels, buffer_length, width_samples, latency_samples, n_samples,
                                     d_indices, capacity, d_counts, stream));
    return SYLDET_OK;
}

int syldet_trigger_rehearse_device(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                   int64_t latency_samples, float *d_track, int64_t n_samples, int64_t track_stride, int64_t *d_indices,
                                   int64_t capacity, int64_t *d_counts, void *hip_stream)
{
    return trigger_rehearse(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_track, n_samples, track_stride, d_indices,
                            capacity, d_counts, (hipStream_t)hip_stream);
}

int syldet_trigger_rehearse_device_s16(syldet_t *h, const uint8_t *d_flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                                       int64_t latency_samples, int16_t *d_track, int64_t n_samples, int64_t track_stride, int64_t *d_indices,
                                       int64_t capacity, int64_t *d_counts, void *hip_stream)
{
    return trigger_rehearse(h, d_flags, n_evals, buffer_length, width_samples, latency_samples, d_track, n_samples, track_stride, d_indices,
                            capacity, d_counts, (hipStream_t)hip_stream);
}

int syldet_trigger(syldet_t *h, const uint8_t *flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples, int64_t latency_samples,
                   float *track, int64_t n_samples, int64_t track_stride)
{
    return trigger_host(h, flags, n_evals, buffer_length, width_samples, latency_samples, track, n_samples, track_stride);
}

int syldet_trigger_s16(syldet_t *h, const uint8_t *flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                       int64_t latency_samples, int16_t *track, int64_t n_samples, int64_t track_stride)
{
    return trigger_host(h, flags, n_evals, buffer_length, width_samples, latency_samples, track, n_samples, track_stride);
}

int syldet_trigger_onsets(syldet_t *h, const uint8_t *flags, int64_t n_evals, int32_t buffer_length, int64_t width_samples,
                          int64_t latency_samples, int64_t n_samples, int64_t *indices, int64_t capacity, int64_t *counts)
{
    if (!counts || capacity < 0 || (capacity > 0 && !indices)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    if (int st = trigger_args(h, flags, n_evals, buffer_length, width_samples, latency_samples, n_samples)) return st;
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    if (int st = trigger_stage_flags(h, flags, n_evals)) return st;
    if (int st = h->d_stage_idx.reserve(std::max<size_t>((size_t)C * (size_t)capacity * sizeof(int64_t), 8))) return st;
    if (int st = h->d_stage_cnt.reserve((size_t)C * sizeof(int64_t))) return st;
    if (int st = syldet_trigger_onsets_device(h, (const uint8_t *)h->d_stage_flags.ptr, n_evals, buffer_length, width_samples, latency_samples,
                                              n_samples, capacity > 0 ? (int64_t *)h->d_stage_idx.ptr : nullptr, capacity,
                                              (int64_t *)h->d_stage_cnt.ptr, h->stream))
        return st;
    if (capacity > 0)
        SYLDET_HIP(hipMemcpyAsync(indices, h->d_stage_idx.ptr, (size_t)C * (size_t)capacity * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipMemcpyAsync(counts, h->d_stage_cnt.ptr, (size_t)C * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

int syldet_trigger_arm(syldet_t *h, int32_t channel, int64_t width_samples)
{
    if (!h || channel < 0 || channel >= h->channels || width_samples < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    trigger_pulse_arm(h->streams[(size_t)channel]->trigger_high, width_samples);
    return SYLDET_OK;
}

int syldet_trigger_render(syldet_t *h, int32_t channel, float *out, int32_t n_frames)
{
    if (!h || channel < 0 || channel >= h->channels || n_frames < 0 || (n_frames > 0 && !out)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    trigger_pulse_render(h->streams[(size_t)channel]->trigger_high, out, n_frames);
    return SYLDET_OK;
}

}  // extern "C"
