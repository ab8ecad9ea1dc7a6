// wav.hpp -- minimal RIFF/WAVE reader for the command line tool: what AVAssetReader + the detector's
// audioSettings (SyllableDetector.swift:19-23: 32-bit float linear PCM) deliver in the reference, for
// the container this image can decode without AVFoundation.  PCM 8/16/24/32-bit and IEEE float
// 32/64-bit, plain or WAVE_FORMAT_EXTENSIBLE, any channel count.  Samples come back frame-major
// (interleaved) as fp32 in [-1, 1): integer PCM is divided by 2^(bits-1), like Core Audio's converter; read_s16 gives 16-bit
// PCM as stored.  write_s16 writes what the Simulator's file writer does for the tool's --simulate (ViewControllerSimulator.swift:187-218:
// 16-bit linear PCM at the network's rate).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace wav {

struct Info {
    int format = 0;          // 1 PCM, 3 IEEE float
    int channels = 0;
    int bits = 0;
    double rate = 0.0;
    int64_t frames = 0;
    int64_t data_offset = 0; // byte offset of the sample data in the file
};

inline uint32_t rd32(const unsigned char *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint16_t rd16(const unsigned char *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// Parses the header; on failure returns false with a reason in `err`.
inline bool probe(const std::string &path, Info &info, std::string &err)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open file"; return false; }
    unsigned char hdr[12];
    if (std::fread(hdr, 1, 12, f) != 12 || std::memcmp(hdr, "RIFF", 4) != 0 || std::memcmp(hdr + 8, "WAVE", 4) != 0) {
        std::fclose(f);
        err = "not a RIFF/WAVE file";
        return false;
    }
    bool have_fmt = false, have_data = false;
    int block_align = 0;
    int64_t pos = 12, data_bytes = 0;
    for (;;) {
        unsigned char ch[8];
        if (std::fseek(f, (long)pos, SEEK_SET) != 0 || std::fread(ch, 1, 8, f) != 8) break;
        const uint32_t size = rd32(ch + 4);
        if (std::memcmp(ch, "fmt ", 4) == 0) {
            unsigned char b[40] = {0};
            const size_t want = size < 40 ? size : 40;
            if (size < 16 || std::fread(b, 1, want, f) != want) { err = "truncated fmt chunk"; break; }
            info.format = rd16(b);
            info.channels = rd16(b + 2);
            info.rate = (double)rd32(b + 4);
            block_align = rd16(b + 12);
            info.bits = rd16(b + 14);
            if (info.format == 0xFFFE && size >= 26) info.format = rd16(b + 24);   // WAVE_FORMAT_EXTENSIBLE: sub-format GUID's first word
            have_fmt = true;
        } else if (std::memcmp(ch, "data", 4) == 0) {
            info.data_offset = pos + 8;
            data_bytes = size;
            have_data = true;
            break;                                     // sample data is the last thing we need
        }
        pos += 8 + (int64_t)size + (size & 1);         // chunks are word aligned
    }
    if (have_fmt && have_data) {
        // a streamed file may carry 0 or 0xFFFFFFFF as its data size: trust the file length then
        std::fseek(f, 0, SEEK_END);
        const int64_t end = (int64_t)std::ftell(f);
        if (data_bytes == 0 || data_bytes == 0xFFFFFFFFll || info.data_offset + data_bytes > end) data_bytes = end - info.data_offset;
    }
    std::fclose(f);
    if (!have_fmt) { if (err.empty()) err = "no fmt chunk"; return false; }
    if (!have_data) { err = "no data chunk"; return false; }
    if (info.channels <= 0) { err = "no audio channels"; return false; }
    const bool pcm = info.format == 1 && (info.bits == 8 || info.bits == 16 || info.bits == 24 || info.bits == 32);
    const bool flt = info.format == 3 && (info.bits == 32 || info.bits == 64);
    if (!pcm && !flt) { err = "unsupported sample format (format tag " + std::to_string(info.format) + ", " + std::to_string(info.bits) + " bits)"; return false; }
    if (block_align != info.channels * info.bits / 8) { err = "inconsistent block alignment"; return false; }
    info.frames = data_bytes / block_align;
    return true;
}

// Reads every frame as interleaved fp32.
inline bool read(const std::string &path, Info &info, std::vector<float> &out, std::string &err)
{
    if (!probe(path, info, err)) return false;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open file"; return false; }
    const size_t n = (size_t)info.frames * (size_t)info.channels, bps = (size_t)info.bits / 8;
    std::vector<unsigned char> raw(n * bps);
    std::fseek(f, (long)info.data_offset, SEEK_SET);
    const size_t got = std::fread(raw.data(), 1, raw.size(), f);
    std::fclose(f);
    if (got != raw.size()) { err = "truncated sample data"; return false; }
    out.resize(n);
    const unsigned char *p = raw.data();
    if (info.format == 3 && info.bits == 32) {
        std::memcpy(out.data(), p, n * 4);
    } else if (info.format == 3) {
        for (size_t i = 0; i < n; i++) { double d; std::memcpy(&d, p + 8 * i, 8); out[i] = (float)d; }
    } else if (info.bits == 16) {
        for (size_t i = 0; i < n; i++) out[i] = (float)(int16_t)rd16(p + 2 * i) * (1.0f / 32768.0f);
    } else if (info.bits == 8) {
        for (size_t i = 0; i < n; i++) out[i] = (float)((int)p[i] - 128) * (1.0f / 128.0f);
    } else if (info.bits == 24) {
        for (size_t i = 0; i < n; i++) {
            const int32_t v = (int32_t)((uint32_t)p[3 * i] << 8 | (uint32_t)p[3 * i + 1] << 16 | (uint32_t)p[3 * i + 2] << 24) >> 8;
            out[i] = (float)v * (1.0f / 8388608.0f);
        }
    } else {
        for (size_t i = 0; i < n; i++) out[i] = (float)((double)(int32_t)rd32(p + 4 * i) * (1.0 / 2147483648.0));
    }
    return true;
}

// Reads every frame of a 16-bit PCM file as interleaved int16, as stored: sample x means x / 32768, the value read() gives
// for it (the *_s16 entry points of the library take these and move half the bytes of fp32).
inline bool read_s16(const std::string &path, Info &info, std::vector<int16_t> &out, std::string &err)
{
    if (!probe(path, info, err)) return false;
    if (info.format != 1 || info.bits != 16) { err = "not 16-bit PCM"; return false; }
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open file"; return false; }
    const size_t n = (size_t)info.frames * (size_t)info.channels;
    std::vector<unsigned char> raw(n * 2);
    std::fseek(f, (long)info.data_offset, SEEK_SET);
    const size_t got = std::fread(raw.data(), 1, raw.size(), f);
    std::fclose(f);
    if (got != raw.size()) { err = "truncated sample data"; return false; }
    out.resize(n);
    for (size_t i = 0; i < n; i++) out[i] = (int16_t)rd16(raw.data() + 2 * i);
    return true;
}

// Reads the header and the sample data as the `data` chunk stores it: frames * channels samples of bits / 8 bytes each, little
// endian, interleaved -- what the library's loads of the files' own bytes take (syldet_recordings_load_pcm_device), with the values
// read() gives.
inline bool read_raw(const std::string &path, Info &info, std::vector<unsigned char> &out, std::string &err)
{
    if (!probe(path, info, err)) return false;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { err = "cannot open file"; return false; }
    out.resize((size_t)info.frames * (size_t)info.channels * ((size_t)info.bits / 8));
    std::fseek(f, (long)info.data_offset, SEEK_SET);
    const size_t got = std::fread(out.data(), 1, out.size(), f);
    std::fclose(f);
    if (got != out.size()) { err = "truncated sample data"; return false; }
    return true;
}

// Writes `frames` frames of `channels` interleaved 16-bit samples as a canonical WAV: the 44-byte header (RIFF, a 16-byte PCM fmt
// chunk, data), little endian.  Refuses what a RIFF size field cannot hold (the file would pass 4 GiB).
inline bool write_s16(const std::string &path, double rate, int channels, int64_t frames, const int16_t *data, std::string &err)
{
    if (channels <= 0 || channels > 32767 || frames < 0 || rate < 1.0 || rate > 4294967295.0) { err = "bad arguments"; return false; }
    const uint64_t bytes = (uint64_t)frames * (uint64_t)channels * 2u;
    if (bytes + 36u > 0xFFFFFFFFull) { err = "too long for a WAV file (4 GiB)"; return false; }
    if (frames > 0 && !data) { err = "bad arguments"; return false; }
    unsigned char h[44];
    auto wr32 = [](unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); p[2] = (unsigned char)(v >> 16); p[3] = (unsigned char)(v >> 24); };
    auto wr16 = [](unsigned char *p, uint32_t v) { p[0] = (unsigned char)v; p[1] = (unsigned char)(v >> 8); };
    const uint32_t r = (uint32_t)(rate + 0.5), align = (uint32_t)channels * 2u;
    std::memcpy(h, "RIFF", 4); wr32(h + 4, (uint32_t)(bytes + 36u)); std::memcpy(h + 8, "WAVEfmt ", 8); wr32(h + 16, 16u);
    wr16(h + 20, 1u); wr16(h + 22, (uint32_t)channels); wr32(h + 24, r); wr32(h + 28, (uint32_t)std::min<uint64_t>((uint64_t)r * align, 0xFFFFFFFFull));
    wr16(h + 32, align); wr16(h + 34, 16u); std::memcpy(h + 36, "data", 4); wr32(h + 40, (uint32_t)bytes);
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) { err = "cannot create file"; return false; }
    bool ok = std::fwrite(h, 1, 44, f) == 44;
    // (little endian on the wire whatever the host: a chunk of samples at a time)
    std::vector<unsigned char> buf;
    const size_t n = (size_t)frames * (size_t)channels, step = 1u << 16;
    for (size_t i = 0; ok && i < n; i += step) {
        const size_t m = n - i < step ? n - i : step;
        buf.resize(2 * m);
        for (size_t k = 0; k < m; k++) { const uint16_t v = (uint16_t)data[i + k]; buf[2 * k] = (unsigned char)v; buf[2 * k + 1] = (unsigned char)(v >> 8); }
        ok = std::fwrite(buf.data(), 1, buf.size(), f) == buf.size();
    }
    if (std::fclose(f) != 0) ok = false;
    if (!ok) err = "write failed";
    return ok;
}

}  // namespace wav
