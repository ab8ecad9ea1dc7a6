// syldet_recordings_levels.cpp -- packed recordings: every recording's level meters (include/syldet.h, "packed recordings: the
// level meters"; kernels_recordings_levels.hip).  The handle (syldet_recordings.hpp) keeps (L, P) and the reading prefix on the
// device, beside the plan's tables, so that a call with the kept pair is launches only.

#include "syldet_recordings.hpp"

namespace {

int geometry_args(int32_t L, int64_t P)
{
    if (int st = buffer_length_arg(L)) return st;
    if (P < 1) return fail(SYLDET_ERR_INVALID_ARGUMENT, "buffers_per_reading must be >= 1");
    return SYLDET_OK;
}

// recording k's M_k = syldet_levels_count(n_k, L, P) readings from first[k] on; first: K + 1 entries, or NULL
int64_t layout(const syldet_recordings_t *r, int32_t L, int64_t P, int64_t *first)
{
    int64_t total = 0;
    for (int k = 0; k < r->plan.K; k++) {
        if (first) first[k] = total;
        total += syldet_levels_count(r->plan.slots[(size_t)k].n_samples, L, P);
    }
    if (first) first[r->plan.K] = total;
    return total;
}

int table_args(const syldet_recordings_t *r, int32_t L, int64_t P, int64_t capacity, int64_t *n_readings)
{
    if (int st = geometry_args(L, P)) return st;
    *n_readings = layout(r, L, P, nullptr);
    if (capacity < *n_readings)
        return fail(SYLDET_ERR_INVALID_ARGUMENT, "capacity " + std::to_string(capacity) + " is below the " + std::to_string(*n_readings) +
                                                     " readings of the recordings (syldet_recordings_levels_layout)");
    return SYLDET_OK;
}

// What both meters begin with on the device.  The kept pair: a call whose (L, P) differs from it (the first always) uploads the
// prefix behind the last levels call.
int levels_begin(syldet_recordings_t *r, int32_t L, int64_t P, hipStream_t stream)
{
    SYLDET_HIP(hipSetDevice(r->bank.device));
    syldet_recordings::Levels &v = r->levels;
    if (!(v.first.kept && v.L == L && v.P == P)) {
        int st = v.first.remake([&]() -> int {
            v.L = L;
            v.P = P;
            const size_t K = (size_t)r->plan.K;
            int64_t *first = v.first.host.data();    // (sized by syldet_recordings_create: no allocation)
            v.desc.n_readings = layout(r, L, P, first);
            for (size_t i = 0; i < K; i++) first[K + 1 + i] = first[(size_t)r->plan.order[i]];   // slot_first, right behind (recordings_blob.hpp)
            return SYLDET_OK;
        });
        if (st) return st;
    }
    v.first.read_on(stream);
    r->h->prof_begin();
    return SYLDET_OK;
}

int levels_impl(syldet_recordings_t *r, const void *d_rows, bool s16, int64_t channel_stride, int32_t L, int64_t P, double *d_mean_square,
                int64_t capacity, hipStream_t stream)
{
    if (!r || !d_rows || !d_mean_square) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = stride_arg(r, channel_stride)) return st;
    int64_t n_readings = 0;
    if (int st = table_args(r, L, P, capacity, &n_readings)) return st;
    if (n_readings == 0) return SYLDET_OK;
    if (int st = levels_begin(r, L, P, stream)) return st;
    if (r->load.desc.tiles >= 2) {
        // (a reading may cross two workgroups of the row: the atomics need +0 underneath)
        KernelTimer t(r->h, stream, "recordings_levels_zero_kernel");
        SYLDET_HIP(launch_recordings_levels_zero(d_mean_square, n_readings, stream));
    }
    KernelTimer t(r->h, stream, "recordings_levels_in_kernel");
    SYLDET_HIP(launch_recordings_levels_in(r->levels.desc, r->bank.channels, d_rows, s16, channel_stride, L, P, d_mean_square, stream));
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
    if (!r || !d_levels || (r->plan.row_evals > 0 && !d_outputs)) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (output < 0 || output >= r->bank.geom.outputs) return fail(SYLDET_ERR_INVALID_ARGUMENT, "output outside [0, outputs)");
    int64_t n_readings = 0;
    if (int st = table_args(r, buffer_length, buffers_per_reading, capacity, &n_readings)) return st;
    if (n_readings == 0) return SYLDET_OK;
    hipStream_t stream = (hipStream_t)hip_stream;
    if (int st = levels_begin(r, buffer_length, buffers_per_reading, stream)) return st;
    KernelTimer t(r->h, stream, "recordings_levels_out_kernel");
    SYLDET_HIP(launch_recordings_levels_out(r->levels.desc, r->bank.channels, d_outputs, r->bank.geom.outputs, output, buffer_length, buffers_per_reading,
                                            (int64_t)r->bank.geom.gap + r->bank.window_length, r->bank.geom.hop, r->bank.time_range, d_levels, stream));
    return SYLDET_OK;
}

}  // extern "C"
