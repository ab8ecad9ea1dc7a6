// syldet_recordings_levels.cpp -- packed recordings: every recording's level meters (include/syldet.h, "packed recordings: the
// level meters"; kernels_recordings_levels.hip).  The handle (syldet_recordings.hpp) keeps (L, P) and the reading prefix on the
// device, beside the plan's tables, so that a call with the kept pair is launches only.

#include "syldet_handle.hpp"
#include "syldet_recordings.hpp"

namespace {

int geometry_args(int32_t L, int64_t P)
{
    if (!levels_buffer_ok(L)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "buffer_length must be a power of two in [8, 4096]");
    if (P < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "buffers_per_reading must be >= 1");
    return SYLDET_OK;
}

// recording k's M_k = syldet_levels_count(n_k, L, P) readings from first[k] on; first: K + 1 entries, or NULL
int64_t layout(const syldet_recordings_t *r, int32_t L, int64_t P, int64_t *first)
{
    int64_t total = 0;
    for (int k = 0; k < r->K; k++) {
        if (first) first[k] = total;
        total += syldet_levels_count(r->slots[(size_t)k].n_samples, L, P);
    }
    if (first) first[r->K] = total;
    return total;
}

int capacity_arg(const syldet_recordings_t *r, int32_t L, int64_t P, int64_t capacity, int64_t *n_readings)
{
    *n_readings = layout(r, L, P, nullptr);
    if (capacity < *n_readings)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " is below the " + std::to_string(*n_readings) +
                                                     " readings of the recordings (syldet_recordings_levels_layout)");
    return SYLDET_OK;
}

// The kept pair: a call whose (L, P) differs from it (the first always) waits for the stream of the last levels call, which may
// still read the prefix, and uploads once with a blocking copy.
int keep_pair(syldet_recordings_t *r, int32_t L, int64_t P)
{
    if (r->levels_L == L && r->levels_P == P) return SYLDET_OK;
    if (r->levels_L != 0) SYLDET_HIP(hipStreamSynchronize(r->levels_last));
    r->levels_L = 0;
    const size_t K = (size_t)r->K;
    int64_t *first = r->levels_host.data();          // (sized by syldet_recordings_create: no allocation)
    r->levels.n_readings = layout(r, L, P, first);
    for (size_t i = 0; i < K; i++) first[K + 1 + i] = first[(size_t)r->order[i]];
    hipError_t e = hipMemcpy(r->d_levels_first, first, r->levels_host.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
    r->levels_L = L;
    r->levels_P = P;
    return SYLDET_OK;
}

int levels_impl(syldet_recordings_t *r, const void *d_rows, bool s16, int64_t channel_stride, int32_t L, int64_t P, double *d_mean_square,
                int64_t capacity, hipStream_t stream)
{
    if (!r || !d_rows || !d_mean_square) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (channel_stride < r->row_samples) return fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride below row_samples");
    if (int st = geometry_args(L, P)) return st;
    int64_t n_readings = 0;
    if (int st = capacity_arg(r, L, P, capacity, &n_readings)) return st;
    if (n_readings == 0) return SYLDET_OK;
    syldet *h = r->h;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_pair(r, L, P)) return st;
    r->levels_last = stream;
    h->prof_begin();
    if (r->load.tiles >= 2) {
        // (a reading may cross two workgroups of the row: the atomics need +0 underneath)
        KernelTimer t(h, stream, "recordings_levels_zero_kernel");
        SYLDET_HIP(launch_recordings_levels_zero(d_mean_square, n_readings, stream));
    }
    KernelTimer t(h, stream, "recordings_levels_in_kernel");
    SYLDET_HIP(launch_recordings_levels_in(r->levels, r->bank.channels, d_rows, s16, channel_stride, L, P, d_mean_square, stream));
    return SYLDET_OK;
}

}  // namespace

extern "C" {

int syldet_recordings_levels_layout(const syldet_recordings_t *r, int32_t buffer_length, int64_t buffers_per_reading, int64_t *reading_first,
                                    int64_t *n_readings)
{
    if (!r || !n_readings) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = geometry_args(buffer_length, buffers_per_reading)) return st;
    *n_readings = layout(r, buffer_length, buffers_per_reading, reading_first);
    return SYLDET_OK;
}

int syldet_recordings_levels_device(syldet_recordings_t *r, const float *d_rows, int64_t channel_stride, int32_t buffer_length,
                                    int64_t buffers_per_reading, double *d_mean_square, int64_t capacity, void *hip_stream)
{
    return levels_impl(r, d_rows, false, channel_stride, buffer_length, buffers_per_reading, d_mean_square, capacity, (hipStream_t)hip_stream);
}

int syldet_recordings_levels_device_s16(syldet_recordings_t *r, const int16_t *d_rows, int64_t channel_stride, int32_t buffer_length,
                                        int64_t buffers_per_reading, double *d_mean_square, int64_t capacity, void *hip_stream)
{
    return levels_impl(r, d_rows, true, channel_stride, buffer_length, buffers_per_reading, d_mean_square, capacity, (hipStream_t)hip_stream);
}

int syldet_recordings_output_levels_device(syldet_recordings_t *r, const float *d_outputs, int32_t output, int32_t buffer_length,
                                           int64_t buffers_per_reading, float *d_levels, int64_t capacity, void *hip_stream)
{
    if (!r || !d_levels || (r->row_evals > 0 && !d_outputs)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (output < 0 || output >= r->bank.geom.outputs) return fail(SYLDET_ERR_INVALID_ARGUMENT, "output outside [0, outputs)");
    if (int st = geometry_args(buffer_length, buffers_per_reading)) return st;
    int64_t n_readings = 0;
    if (int st = capacity_arg(r, buffer_length, buffers_per_reading, capacity, &n_readings)) return st;
    if (n_readings == 0) return SYLDET_OK;
    syldet *h = r->h;
    hipStream_t stream = (hipStream_t)hip_stream;
    SYLDET_HIP(hipSetDevice(r->bank.device));
    if (int st = keep_pair(r, buffer_length, buffers_per_reading)) return st;
    r->levels_last = stream;
    h->prof_begin();
    KernelTimer t(h, stream, "recordings_levels_out_kernel");
    SYLDET_HIP(launch_recordings_levels_out(r->levels, r->bank.channels, d_outputs, r->bank.geom.outputs, output, buffer_length, buffers_per_reading,
                                            (int64_t)r->bank.geom.gap + r->bank.window_length, r->bank.geom.hop, r->bank.time_range, d_levels, stream));
    return SYLDET_OK;
}

}  // extern "C"
