// syldet_pcm.cpp -- the files' own sample formats on the host (include/syldet.h, "packed recordings: the files' own sample
// formats"): syldet_pcm_sample_bytes and syldet_pcm_decode, the values the device loads (kernels_recordings_pcm.hip,
// kernels_recordings_sinc.hip) are held to, and syldet_pcm_check_sources, the loads' refusals of a byte source without a handle.
// The arithmetic is pcm_values.hpp's, the kernels' own text; the checks are syldet_recordings.hpp's, the loads' own.
#include "syldet_recordings.hpp"

extern "C" {

int32_t syldet_pcm_sample_bytes(int32_t format) { return sd::pcm_sample_bytes(format); }

int syldet_pcm_decode(int32_t format, const void *bytes, int64_t n, int64_t byte_step, float *out)
{
    const int size = sd::pcm_sample_bytes(format);
    if (size == 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "an unknown sample format");
    if (n < 0 || (n > 0 && (!bytes || !out))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "a NULL array or a negative count");
    if (byte_step < size) return fail(SYLDET_ERR_INVALID_ARGUMENT, "byte_step below the bytes of a sample");
    const unsigned char *p = (const unsigned char *)bytes;
    int64_t i = 0;
    if (byte_step == size)
        for (; i + 4 <= n; i += 4) sd::pcm_group4(format, p + i * byte_step, out + i);
    for (; i < n; i++) out[i] = sd::pcm_value(format, p + i * byte_step);
    return SYLDET_OK;
}

int syldet_pcm_check_sources(const void *src, int64_t src_bytes, const int64_t *src_byte_offset, const int32_t *src_byte_step,
                             const int32_t *src_format, const int64_t *n_samples, int32_t n_recordings)
{
    const int K = n_recordings;
    if (K < 0 || (K > 0 && (!src || !src_byte_offset || !src_format || !n_samples))) return fail(SYLDET_ERR_INVALID_ARGUMENT, "NULL argument");
    if (int st = source_args(K, src_byte_offset, src_byte_step)) return st;
    const PcmSrc pcm{src_bytes, src_format};
    return pcm_args(K, src, pcm, src_byte_offset, src_byte_step, [&](int k) { return n_samples[k]; });
}

}  // extern "C"
