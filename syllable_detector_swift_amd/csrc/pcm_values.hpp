// pcm_values.hpp -- what a sample of a file means, format by format (include/syldet.h, "packed recordings: the files' own sample
// formats"): one text for the host (syldet_pcm_decode, syldet_pcm.cpp), the kernels that load packed recordings from the files' own
// bytes (kernels_recordings_pcm.hip, kernels_recordings_sinc.hip) and a stand-alone program (tests/cpp/pcm_values_test.cpp).  The
// reference has AVFoundation deliver every file as 32-bit float linear PCM (audioSettings, Common/SyllableDetector.swift:19-23);
// these are the values the tool's WAV reader (cli/wav.hpp) makes of the same bytes.  Little endian only.
//   pcm_sample_bytes   the bytes of one sample, 0 for an unknown format
//   pcm_value          one sample at any address its format allows (U8, S24: any; the others: a multiple of their size)
//   pcm_group4         four contiguous samples, read as wide as their address allows and never past their last byte
// No statement here can contract (a conversion and one multiplication by a power of two a sample); the files that include it are
// compiled with -ffp-contract=off all the same (see the Makefile).
#pragma once

#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define SD_PCM_FN __host__ __device__ __forceinline__
#else
#define SD_PCM_FN inline
#endif

namespace sd {

// SYLDET_PCM_* of include/syldet.h (0: no format -- a source counted in elements)
enum { kPcmU8 = 1, kPcmS16 = 2, kPcmS24 = 3, kPcmS32 = 4, kPcmF32 = 5, kPcmF64 = 6 };

SD_PCM_FN int pcm_sample_bytes(int format)
{
    switch (format) {
    case kPcmU8: return 1;
    case kPcmS16: return 2;
    case kPcmS24: return 3;
    case kPcmS32: case kPcmF32: return 4;
    case kPcmF64: return 8;
    default: return 0;
    }
}

// sizeof(W) bytes at p, a multiple of alignof(W) on the device (one access); any address on the host
template <class W>
SD_PCM_FN W pcm_read(const unsigned char *p)
{
#ifdef __HIP_DEVICE_COMPILE__
    return *reinterpret_cast<const W *>(p);
#else
    W w;
    std::memcpy(&w, p, sizeof w);
    return w;
#endif
}

struct alignas(4) PcmWords3 { uint32_t w[3]; };    // a group of four S24 samples
struct alignas(16) PcmWords4 { uint32_t w[4]; };

SD_PCM_FN float pcm_bits_f32(uint32_t b)
{
    float f;
    std::memcpy(&f, &b, 4);                         // (the bits, NaN payloads included)
    return f;
}
SD_PCM_FN float pcm_f64(uint32_t lo, uint32_t hi)
{
    const uint64_t b = (uint64_t)hi << 32 | lo;
    double d;
    std::memcpy(&d, &b, 8);
    return (float)d;                                // round to nearest even; an fp32 subnormal stays one
}
SD_PCM_FN float pcm_s24(uint32_t v) { return (float)((int32_t)(v << 8) >> 8) * (1.0f / 8388608.0f); }    // v: the sample in bits 0-23
SD_PCM_FN float pcm_s32(uint32_t v) { return (float)(int32_t)v * (1.0f / 2147483648.0f); }
SD_PCM_FN float pcm_s16(uint32_t v) { return (float)(int16_t)(uint16_t)v * (1.0f / 32768.0f); }         // v: the sample in bits 0-15
SD_PCM_FN float pcm_u8(uint32_t v) { return (float)((int)(v & 0xffu) - 128) * (1.0f / 128.0f); }

// One sample.  S24 and U8 byte by byte; the others one access of their own size.
SD_PCM_FN float pcm_value(int format, const unsigned char *p)
{
    switch (format) {
    case kPcmU8: return pcm_u8(p[0]);
    case kPcmS16: return pcm_s16(pcm_read<uint16_t>(p));
    case kPcmS24: return pcm_s24((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16);
    case kPcmS32: return pcm_s32(pcm_read<uint32_t>(p));
    case kPcmF32: return pcm_bits_f32(pcm_read<uint32_t>(p));
    case kPcmF64: {
        const uint64_t b = pcm_read<uint64_t>(p);
        return pcm_f64((uint32_t)b, (uint32_t)(b >> 32));
    }
    default: return 0.0f;
    }
}

// Four contiguous samples at p (sample j at p + j pcm_sample_bytes(format)), p as pcm_value takes it.  Exactly the 4, 8, 12, 16 or
// 32 bytes of the four samples are read: U8 4 bytes at once, S16 8 at once or as two words, S24 12 at once (three words), S32 and F32
// 16 at once, as two pairs or as four words, F64 32 as two 16s or four 8s -- each as the address allows; U8 and S24 off a multiple
// of 4 and S16 off one go sample by sample.
SD_PCM_FN void pcm_group4(int format, const unsigned char *p, float *out)
{
    const unsigned a = (unsigned)(uintptr_t)p;
    uint32_t w[8];
    switch (format) {
    case kPcmU8:
        if (a & 3u) break;
        w[0] = pcm_read<uint32_t>(p);
        for (int j = 0; j < 4; j++) out[j] = pcm_u8(w[0] >> (8 * j));
        return;
    case kPcmS16:
        if (a & 3u) break;
        if ((a & 7u) == 0) {
            const uint64_t b = pcm_read<uint64_t>(p);
            w[0] = (uint32_t)b;
            w[1] = (uint32_t)(b >> 32);
        } else {
            w[0] = pcm_read<uint32_t>(p);
            w[1] = pcm_read<uint32_t>(p + 4);
        }
        for (int j = 0; j < 4; j++) out[j] = pcm_s16(w[j >> 1] >> (16 * (j & 1)));
        return;
    case kPcmS24: {
        if (a & 3u) break;
        const PcmWords3 t = pcm_read<PcmWords3>(p);
        out[0] = pcm_s24(t.w[0]);
        out[1] = pcm_s24(t.w[0] >> 24 | t.w[1] << 8);
        out[2] = pcm_s24(t.w[1] >> 16 | t.w[2] << 16);
        out[3] = pcm_s24(t.w[2] >> 8);
        return;
    }
    case kPcmS32:
    case kPcmF32:
        if ((a & 15u) == 0) {
            const PcmWords4 t = pcm_read<PcmWords4>(p);
            for (int j = 0; j < 4; j++) w[j] = t.w[j];
        } else if ((a & 7u) == 0) {
            for (int j = 0; j < 2; j++) {
                const uint64_t b = pcm_read<uint64_t>(p + 8 * j);
                w[2 * j] = (uint32_t)b;
                w[2 * j + 1] = (uint32_t)(b >> 32);
            }
        } else {
            for (int j = 0; j < 4; j++) w[j] = pcm_read<uint32_t>(p + 4 * j);
        }
        for (int j = 0; j < 4; j++) out[j] = format == kPcmF32 ? pcm_bits_f32(w[j]) : pcm_s32(w[j]);
        return;
    case kPcmF64:
        if ((a & 15u) == 0) {
            for (int j = 0; j < 2; j++) {
                const PcmWords4 t = pcm_read<PcmWords4>(p + 16 * j);
                for (int i = 0; i < 4; i++) w[4 * j + i] = t.w[i];
            }
        } else {
            for (int j = 0; j < 4; j++) {
                const uint64_t b = pcm_read<uint64_t>(p + 8 * j);
                w[2 * j] = (uint32_t)b;
                w[2 * j + 1] = (uint32_t)(b >> 32);
            }
        }
        for (int j = 0; j < 4; j++) out[j] = pcm_f64(w[2 * j], w[2 * j + 1]);
        return;
    default:
        break;
    }
    const int size = pcm_sample_bytes(format);
    for (int j = 0; j < 4; j++) out[j] = pcm_value(format, p + j * size);
}

}  // namespace sd
