// syldet_levels.cpp -- the host side of the level meters: the library's sum of squares (what vDSP_svesq is to
// Processor.swift:111-113, with the summation order fixed) for the streaming appends, the count of readings, and the meters'
// entry points (Processor.swift:111-113, :138, :158-184; kernels_levels.hip).
//
// Compiled with -ffp-contract=off (see the Makefile): every square and every addition rounds to fp32 on its own.  (The entry
// points check arguments, stage data and launch kernels: no arithmetic of theirs could contract.)

#include "syldet_handle.hpp"

namespace sd {

namespace {

inline float sample_of(float x) { return x; }
inline float sample_of(int16_t x) { return (float)x * (1.0f / 32768.0f); }   // exact

// The balanced binary tree over next_pow2(n) slots, in index order, slots past n holding +0: a binary counter of finished
// subtrees (level l holds the sum of 2^l squares when bit l of the count is set).  What is left at the end is summed from the
// lowest level up: the missing right halves are +0, and s + (+0) == s (a square is never -0).
template <class T>
float tree(const T *x, int64_t n, int64_t step)
{
    float level[64];
    for (int64_t i = 0; i < n; i++) {
        const float v = sample_of(x[i * step]);
        float s = v * v;
        int l = 0;
        for (int64_t bits = i; bits & 1; bits >>= 1) s = level[l++] + s;
        level[l] = s;
    }
    float s = 0.0f;
    bool any = false;
    for (int l = 0; l < 63; l++)
        if ((n >> l) & 1) {
            s = any ? level[l] + s : level[l];
            any = true;
        }
    return s;
}

}  // namespace

float sum_squares_tree(const float *x, int64_t n, int64_t step) { return tree(x, n, step); }
float sum_squares_tree(const int16_t *x, int64_t n, int64_t step) { return tree(x, n, step); }

}  // namespace sd

static int levels_geometry_args(int32_t L, int64_t P)
{
    if (int st = buffer_length_arg(L)) return st;
    if (P < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "buffers_per_reading must be >= 1");
    return SYLDET_OK;
}

static int levels_args(const syldet *h, const void *samples, int64_t n_samples, int64_t stride, int32_t L, int64_t P, const void *result)
{
    if (!h || !samples || !result) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_samples < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "negative size");
    if (stride < n_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride < n_samples");
    return levels_geometry_args(L, P);
}

static int output_levels_args(const syldet *h, const void *outputs, int64_t n_evals, int32_t output, int64_t n_samples, int32_t L, int64_t P,
                              const void *levels)
{
    if (!h || !outputs || !levels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_evals < 0 || n_samples < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "negative size");
    if (output < 0 || output >= h->geom.outputs) return fail(SYLDET_ERR_INVALID_ARGUMENT, "output outside [0, outputs)");
    return levels_geometry_args(L, P);
}

static int levels_on_stream(syldet *h, Samples x, int64_t n_samples, int64_t stride, int32_t L, int64_t P, double *d_mean_square,
                            hipStream_t stream, bool begin = true)
{
    if (n_samples == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    if (int st = h->d_levels_part.reserve(levels_scratch_bytes(n_samples, C, L, x.s16))) return st;
    if (begin) h->prof_begin();
    bool needs_fold = false;
    {
        KernelTimer t(h, stream, "levels_in_kernel");
        SYLDET_HIP(launch_levels_in(x.p, x.s16, C, n_samples, stride, L, P, d_mean_square, h->d_levels_part.ptr, stream, &needs_fold));
    }
    if (needs_fold) {
        KernelTimer t(h, stream, "levels_fold_kernel");
        SYLDET_HIP(launch_levels_fold(h->d_levels_part.ptr, x.s16, C, n_samples, L, P, d_mean_square, stream));
    }
    return SYLDET_OK;
}

// frames -> the handle's planar scratch (the caller's sample width, rows of whole 16-byte groups), then the planar kernel
static int levels_interleaved(syldet *h, Samples x, int64_t n_frames, int32_t total_channels, int32_t L, int64_t P, double *d_mean_square,
                              hipStream_t stream)
{
    if (int st = interleaved_args(h, n_frames, total_channels)) return st;
    if (!x.p || !d_mean_square) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = levels_geometry_args(L, P)) return st;
    if (n_frames == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    const int64_t ws = (n_frames + 7) & ~(int64_t)7;
    if (int st = h->d_planar.reserve((size_t)C * (size_t)ws * (x.s16 ? sizeof(int16_t) : sizeof(float)))) return st;
    h->prof_begin();
    {
        KernelTimer t(h, stream, x.s16 ? "deinterleave_s16_kernel" : "deinterleave_kernel");
        if (x.s16) SYLDET_HIP(launch_deinterleave_s16((const int16_t *)x.p, n_frames, C, C, (int16_t *)h->d_planar.ptr, ws, stream));
        else SYLDET_HIP(launch_deinterleave((const float *)x.p, n_frames, C, 0, C, (float *)h->d_planar.ptr, ws, stream));
    }
    return levels_on_stream(h, Samples(h->d_planar.ptr, x.s16), n_frames, ws, L, P, d_mean_square, stream, false);
}

template <class T>
static int levels_host(syldet *h, const T *samples, int64_t n_samples, int64_t stride, int32_t L, int64_t P, double *rms)
{
    if (int st = levels_args(h, samples, n_samples, stride, L, P, rms)) return st;
    if (n_samples == 0) return SYLDET_OK;
    std::lock_guard<std::mutex> staging(h->pump_mu);   // the staging buffers and h->stream: one user at a time
    SYLDET_HIP(hipSetDevice(h->device));
    const int C = h->channels;
    const int64_t ws = (n_samples + 7) & ~(int64_t)7;  // rows of whole 16-byte groups
    const size_t n = (size_t)C * (size_t)syldet_levels_count(n_samples, L, P);
    if (int st = h->d_stage_in.reserve((size_t)C * (size_t)ws * sizeof(T))) return st;
    if (int st = h->d_levels.reserve(n * sizeof(double))) return st;
    SYLDET_HIP(hipMemcpy2DAsync(h->d_stage_in.ptr, (size_t)ws * sizeof(T), samples, (size_t)stride * sizeof(T), (size_t)n_samples * sizeof(T),
                                (size_t)C, hipMemcpyHostToDevice, h->stream));
    if (int st = levels_on_stream(h, Samples(h->d_stage_in.ptr, sizeof(T) == 2), n_samples, ws, L, P, (double *)h->d_levels.ptr, h->stream)) return st;
    SYLDET_HIP(hipMemcpyAsync(rms, h->d_levels.ptr, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < n; i++) rms[i] = std::sqrt(rms[i]);   // Processor.swift:168
    return SYLDET_OK;
}

// readStatAndReset (SummaryStat.swift): the value and nothing written any more, or no value
static int read_meter(syldet *h, int32_t channel, bool input, double *value, int32_t *has_value)
{
    if (!h || !value || !has_value || channel < 0 || channel >= h->channels) return fail(SYLDET_ERR_INVALID_ARGUMENT, "bad argument");
    *value = 0.0;
    *has_value = 0;
    if (!h->meters_on.load(std::memory_order_acquire)) return SYLDET_OK;
    syldet::Meter &m = *h->meters[(size_t)channel];
    std::lock_guard<std::mutex> lock(m.mu);
    bool &has = input ? m.in_has : m.out_has;
    if (has) {
        *value = input ? std::sqrt(m.in_cur) : m.out_cur;        // Processor.swift:168: the RMS
        *has_value = 1;
        has = false;
    }
    return SYLDET_OK;
}

extern "C" {

float syldet_sum_squares(const float *x, int64_t n)
{
    if (!x || n <= 0) return 0.0f;
    return sd::sum_squares_tree(x, n, 1);
}

int64_t syldet_levels_count(int64_t n_samples, int32_t buffer_length, int64_t buffers_per_reading)
{
    if (n_samples < 0 || !sd::levels_buffer_ok(buffer_length) || buffers_per_reading < 1) return -1;
    const int64_t B = n_samples / buffer_length + (n_samples % buffer_length != 0);
    return B / buffers_per_reading + (B % buffers_per_reading != 0);
}

int syldet_levels_device(syldet_t *h, const float *d_samples, int64_t n_samples, int64_t channel_stride, int32_t buffer_length,
                         int64_t buffers_per_reading, double *d_mean_square, void *hip_stream)
{
    if (int st = levels_args(h, d_samples, n_samples, channel_stride, buffer_length, buffers_per_reading, d_mean_square)) return st;
    return levels_on_stream(h, d_samples, n_samples, channel_stride, buffer_length, buffers_per_reading, d_mean_square, (hipStream_t)hip_stream);
}

int syldet_levels_device_s16(syldet_t *h, const int16_t *d_samples, int64_t n_samples, int64_t channel_stride, int32_t buffer_length,
                             int64_t buffers_per_reading, double *d_mean_square, void *hip_stream)
{
    if (int st = levels_args(h, d_samples, n_samples, channel_stride, buffer_length, buffers_per_reading, d_mean_square)) return st;
    return levels_on_stream(h, Samples(d_samples, true), n_samples, channel_stride, buffer_length, buffers_per_reading, d_mean_square,
                            (hipStream_t)hip_stream);
}

int syldet_levels_interleaved_device(syldet_t *h, const float *d_interleaved, int64_t n_frames, int32_t total_channels, int32_t buffer_length,
                                     int64_t buffers_per_reading, double *d_mean_square, void *hip_stream)
{
    return levels_interleaved(h, d_interleaved, n_frames, total_channels, buffer_length, buffers_per_reading, d_mean_square, (hipStream_t)hip_stream);
}

int syldet_levels_interleaved_device_s16(syldet_t *h, const int16_t *d_interleaved, int64_t n_frames, int32_t total_channels,
                                         int32_t buffer_length, int64_t buffers_per_reading, double *d_mean_square, void *hip_stream)
{
    return levels_interleaved(h, Samples(d_interleaved, true), n_frames, total_channels, buffer_length, buffers_per_reading, d_mean_square,
                              (hipStream_t)hip_stream);
}

int syldet_levels_eval_range(const syldet_t *h, int64_t n_samples, int64_t n_evals, int32_t buffer_length, int64_t buffers_per_reading,
                             int64_t reading, int64_t *first, int64_t *count)
{
    if (!h || !first || !count) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (n_samples < 0 || n_evals < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "negative size");
    if (int st = levels_geometry_args(buffer_length, buffers_per_reading)) return st;
    const int64_t M = syldet_levels_count(n_samples, buffer_length, buffers_per_reading);
    if (reading < 0 || reading >= M) return fail(SYLDET_ERR_INVALID_ARGUMENT, "reading outside [0, syldet_levels_count)");
    // (reading < M: reading * P < B <= n_samples, and the products stay inside 64 bits)
    const int64_t B = n_samples / buffer_length + (n_samples % buffer_length != 0);
    const int64_t PL = std::min(buffers_per_reading, B) * buffer_length;
    const int64_t e0 = std::min(count_evals(h, std::min(reading * PL, n_samples)), n_evals);
    const int64_t e1 = std::min(count_evals(h, std::min((reading + 1) * PL, n_samples)), n_evals);
    *first = e0;
    *count = e1 - e0;
    return SYLDET_OK;
}

int syldet_output_levels_device(syldet_t *h, const float *d_outputs, int64_t n_evals, int32_t output, int64_t n_samples, int32_t buffer_length,
                                int64_t buffers_per_reading, float *d_levels, void *hip_stream)
{
    if (int st = output_levels_args(h, d_outputs, n_evals, output, n_samples, buffer_length, buffers_per_reading, d_levels)) return st;
    if (n_samples == 0) return SYLDET_OK;
    SYLDET_HIP(hipSetDevice(h->device));
    hipStream_t stream = (hipStream_t)hip_stream;
    h->prof_begin();
    KernelTimer t(h, stream, "levels_out_kernel");
    SYLDET_HIP(launch_levels_out(d_outputs, n_evals, h->geom.outputs, output, h->channels, n_samples, buffer_length, buffers_per_reading,
                                 (int64_t)h->geom.gap + h->cfg.view.window_length, h->geom.hop, h->cfg.view.time_range, d_levels, stream));
    return SYLDET_OK;
}

int syldet_levels(syldet_t *h, const float *samples, int64_t n_samples, int64_t channel_stride, int32_t buffer_length,
                  int64_t buffers_per_reading, double *rms)
{
    return levels_host(h, samples, n_samples, channel_stride, buffer_length, buffers_per_reading, rms);
}

int syldet_levels_s16(syldet_t *h, const int16_t *samples, int64_t n_samples, int64_t channel_stride, int32_t buffer_length,
                      int64_t buffers_per_reading, double *rms)
{
    return levels_host(h, samples, n_samples, channel_stride, buffer_length, buffers_per_reading, rms);
}

int syldet_output_levels(syldet_t *h, const float *outputs, int64_t n_evals, int32_t output, int64_t n_samples, int32_t buffer_length,
                         int64_t buffers_per_reading, float *levels)
{
    if (int st = output_levels_args(h, outputs, n_evals, output, n_samples, buffer_length, buffers_per_reading, levels)) return st;
    if (n_samples == 0) return SYLDET_OK;
    std::lock_guard<std::mutex> staging(h->pump_mu);
    SYLDET_HIP(hipSetDevice(h->device));
    const size_t out_bytes = (size_t)h->channels * (size_t)n_evals * (size_t)h->geom.outputs * sizeof(float);
    const size_t n = (size_t)h->channels * (size_t)syldet_levels_count(n_samples, buffer_length, buffers_per_reading);
    if (int st = h->d_stage_out.reserve(std::max<size_t>(out_bytes, 4))) return st;
    if (int st = h->d_levels.reserve(n * sizeof(float))) return st;
    if (out_bytes) SYLDET_HIP(hipMemcpyAsync(h->d_stage_out.ptr, outputs, out_bytes, hipMemcpyHostToDevice, h->stream));
    if (int st = syldet_output_levels_device(h, (const float *)h->d_stage_out.ptr, n_evals, output, n_samples, buffer_length, buffers_per_reading,
                                             (float *)h->d_levels.ptr, h->stream))
        return st;
    SYLDET_HIP(hipMemcpyAsync(levels, h->d_levels.ptr, n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    SYLDET_HIP(hipStreamSynchronize(h->stream));
    return SYLDET_OK;
}

int syldet_meters_enable(syldet_t *h, int enable)
{
    if (!h) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL handle");
    try {
        if (h->meters.empty()) {
            std::vector<std::unique_ptr<syldet::Meter>> m((size_t)h->channels);
            for (auto &p : m) p.reset(new syldet::Meter());
            h->meters = std::move(m);
        }
    } catch (const std::bad_alloc &) {
        return fail(SYLDET_ERR_OUT_OF_MEMORY, "out of memory");
    }
    for (auto &m : h->meters) {
        std::lock_guard<std::mutex> lock(m->mu);
        m->in_has = m->out_has = false;
    }
    h->meters_on.store(enable != 0, std::memory_order_release);
    return SYLDET_OK;
}

int syldet_input_level(syldet_t *h, int32_t channel, double *rms, int32_t *has_value) { return read_meter(h, channel, true, rms, has_value); }
int syldet_output_level(syldet_t *h, int32_t channel, double *level, int32_t *has_value) { return read_meter(h, channel, false, level, has_value); }

}  // extern "C"
