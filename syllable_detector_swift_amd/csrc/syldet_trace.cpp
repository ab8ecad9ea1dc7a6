// syldet_trace.cpp -- the Simulator's output track (ViewControllerSimulator.swift:251-344; kernels_trace.hip)

#include "syldet_handle.hpp"

static int trace_args(const syldet *h, const void *outputs, int64_t n_evals, int32_t output, const void *trace, int64_t n_samples,
                      int64_t trace_stride)
{
    if (!h || !outputs || !trace) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_evals < 0 || n_samples < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "negative size");
    if (trace_stride < n_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "trace_stride < n_samples");
    if (output < 0 || output >= h->geom.outputs) return fail(SYLDET_ERR_INVALID_ARGUMENT, "output outside [0, outputs)");
    return SYLDET_OK;
}

// Float(thresholds[k]) of every channel's own network on the device: made on the first trace of output k, kept by the handle
int sd::trace_thresholds(syldet *h, int k, const float **out)
{
    try {
        if (h->d_trace_thr.empty()) h->d_trace_thr.resize((size_t)h->geom.outputs);
        DeviceBuffer &b = h->d_trace_thr[(size_t)k];
        if (!b.ptr) {
            const int C = h->channels, n_out = h->geom.outputs;
            std::vector<float> t((size_t)C);
            for (int c = 0; c < C; c++)
                t[(size_t)c] = (float)(h->chan_thr.empty() ? h->cfg.view.thresholds[k] : h->chan_thr[(size_t)c * (size_t)n_out + (size_t)k]);
            if (int st = b.reserve((size_t)C * sizeof(float))) return st;
            if (hipError_t e = hipMemcpy(b.ptr, t.data(), (size_t)C * sizeof(float), hipMemcpyHostToDevice)) {
                b.release();
                return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
            }
        }
        *out = (const float *)b.ptr;
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    return SYLDET_OK;
}

// T: float or int16_t rows [C][stride]; frames: int16 [n_samples][C] instead
template <class T>
static int trace_on_stream(syldet *h, const float *d_outputs, int64_t n_evals, int32_t k, T *d_trace, int64_t n_samples, int64_t stride,
                           bool frames, hipStream_t stream)
{
    if (n_samples == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(h->device));
    const float *thr = nullptr;
    if (int st = trace_thresholds(h, k, &thr)) return st;
    const int C = h->channels, n_out = h->geom.outputs;
    const int64_t D = h->geom.first_index, hop = h->geom.hop;
    h->prof_begin();
    if constexpr (sizeof(T) == 2) {
        if (frames) {
            KernelTimer t(h, stream, C == 1 ? "trace_kernel" : "trace_interleaved_s16_kernel");   // (one channel: launch_trace_interleaved_s16 runs the planar kernel)
            SYLDET_HIP(launch_trace_interleaved_s16(d_outputs, n_evals, n_out, k, thr, C, d_trace, n_samples, D, hop, stream));
            return SYLDET_OK;
        }
        KernelTimer t(h, stream, "trace_kernel");
        SYLDET_HIP(launch_trace_s16(d_outputs, n_evals, n_out, k, thr, C, d_trace, n_samples, stride, D, hop, stream));
    } else {
        KernelTimer t(h, stream, "trace_kernel");
        SYLDET_HIP(launch_trace(d_outputs, n_evals, n_out, k, thr, C, d_trace, n_samples, stride, D, hop, stream));
    }
    return SYLDET_OK;
}

template <class T>
static int trace_host(syldet *h, const float *outputs, int64_t n_evals, int32_t output, T *trace, int64_t n_samples, int64_t trace_stride)
{
    if (int st = trace_args(h, outputs, n_evals, output, trace, n_samples, trace_stride)) return st;
    if (n_samples == 0) return SYLDET_OK;
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    const size_t out_bytes = (size_t)C * (size_t)n_evals * (size_t)h->geom.outputs * sizeof(float);
    const int64_t ws = (n_samples + 7) & ~(int64_t)7;  // rows of whole 16-byte groups
    if (int st = h->d_stage_out.reserve(std::max<size_t>(out_bytes, 4))) return st;
    if (int st = h->d_trace.reserve((size_t)C * (size_t)ws * sizeof(T))) return st;
    if (out_bytes) SYLDET_HIP(hipMemcpyAsync(h->d_stage_out.ptr, outputs, out_bytes, hipMemcpyHostToDevice, h->stream));
    if (int st = trace_on_stream(h, (const float *)h->d_stage_out.ptr, n_evals, output, (T *)h->d_trace.ptr, n_samples, ws, false, h->stream)) return st;
    SYLDET_HIP(hipMemcpy2DAsync(trace, (size_t)trace_stride * sizeof(T), h->d_trace.ptr, (size_t)ws * sizeof(T), (size_t)n_samples * sizeof(T),
                                (size_t)C, hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

extern "C" {

int syldet_trace_device(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output, float *d_trace, int64_t n_samples,
                        int64_t trace_stride, void *hip_stream)
{
    if (int st = trace_args(h, d_outputs, n_evals, output, d_trace, n_samples, trace_stride)) return st;
    return trace_on_stream(h, d_outputs, n_evals, output, d_trace, n_samples, trace_stride, false, (hipStream_t)hip_stream);
}

int syldet_trace_device_s16(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output, int16_t *d_trace, int64_t n_samples,
                            int64_t trace_stride, void *hip_stream)
{
    if (int st = trace_args(h, d_outputs, n_evals, output, d_trace, n_samples, trace_stride)) return st;
    return trace_on_stream(h, d_outputs, n_evals, output, d_trace, n_samples, trace_stride, false, (hipStream_t)hip_stream);
}

int syldet_trace_interleaved_device_s16(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output, int16_t *d_frames,
                                        int64_t n_samples, void *hip_stream)
{
    if (int st = trace_args(h, d_outputs, n_evals, output, d_frames, n_samples, n_samples)) return st;
    return trace_on_stream(h, d_outputs, n_evals, output, d_frames, n_samples, n_samples, true, (hipStream_t)hip_stream);
}

int syldet_trace(syldet_t *h, const float *outputs, int64_t n_evals, int32_t output, float *trace, int64_t n_samples, int64_t trace_stride)
{
    return trace_host(h, outputs, n_evals, output, trace, n_samples, trace_stride);
}

int syldet_trace_s16(syldet_t *h, const float *outputs, int64_t n_evals, int32_t output, int16_t *trace, int64_t n_samples,
                     int64_t trace_stride)
{
    return trace_host(h, outputs, n_evals, output, trace, n_samples, trace_stride);
}

}  // extern "C"
