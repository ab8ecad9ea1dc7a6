// syldet_recordings.hpp -- the packed-recordings handle (struct syldet_recordings) for the host files that share it:
// syldet_recordings.cpp (the plan, the loads, the events), syldet_recordings_tracks.cpp (the per-sample tracks) and
// syldet_recordings_levels.cpp (the level meters).  Not installed.
#pragma once

#include "pcm_values.hpp"
#include "syldet_handle.hpp"

namespace sd {

// A table on the device that stays valid while its key is unchanged.  The owner compares the key: a call with the kept key is
// launches only, one with another key (the first always) re-makes the table; every call notes the stream that reads it.
template <class T>
struct KeptTable {
    std::vector<T> host;             // what one copy uploads (sized by syldet_recordings_create: no call allocates)
    T *dev = nullptr;                // (inside the handle's block)
    bool kept = false;
    hipStream_t last = nullptr;      // the stream of the last call that may still read dev

    // Waits for the last reader, has fill() make `host` (its status ends the call), uploads once with a blocking copy -- the one
    // copy include/syldet.h speaks of -- and is kept only once that succeeded.  also: wait although nothing is kept (the last
    // call read a table beside this one).
    template <class Fill>
    int remake(Fill fill, bool also = false)
    {
        if (kept || also) SYLDET_HIP(hipStreamSynchronize(last));
        kept = false;
        if (int st = fill()) return st;
        hipError_t e = hipMemcpy(dev, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(SYLDET_ERR_DEVICE, std::string("hipMemcpy: ") + hipGetErrorString(e));
        kept = true;
        return SYLDET_OK;
    }
    void read_on(hipStream_t stream) { last = stream; }
};

}  // namespace sd

// Each group: its key (where the table is not its own key), its kept table, its descriptor.
struct syldet_recordings {
    syldet_t *h = nullptr;                   // the bank (it outlives this handle): its thresholds and its profile
    sd::BankInfo bank{};
    sd::DeviceBuffer blob;                   // every table below in one block (recordings_blob.hpp)

    struct Plan {                            // made by syldet_recordings_create, never changed
        int K = 0;
        std::vector<syldet_slot_t> slots;    // [K] the caller's order
        int64_t row_samples = 0, row_evals = 0;
        double fill = 0.0;
        std::vector<int32_t> order;          // order[i] = the recording of table entry i (the slots sorted by (row, offset))
        std::vector<int32_t> row_begin;      // [C + 1] the table's rows
        const sd::RecEventDev *d_events = nullptr;
    } plan;

    // The plain load (syldet_recordings_load_device*).  Its table holds whole RecSlotDev entries, which the track and level kernels
    // read as well (RecLoadDesc): re-making it under them is sound only because the fields they read, offset and n_samples, are
    // rewritten with the values they hold already.
    struct Load {
        sd::KeptTable<sd::RecSlotDev> table; // [K] in `order`; on the device without sources from create on
        sd::RecLoadDesc desc{};
    } load;

    // The converting load (syldet_recordings_load_sinc_device*): tables of its own, so that plain and converting loads may take
    // turns on one handle.
    struct Sinc {
        int32_t Z = 0;
        double beta = 0.0, rho = 0.0;
        sd::KeptTable<char> table;           // RecSincDev [K] in `order` | workgroup prefixes [K + C]
        size_t wg_at = 0;                    // where the prefixes begin in it
        sd::RecSincDesc desc{};
    } sinc;

    // The per-sample tracks (syldet_recordings_tracks.cpp): tables apart from the loads', so loads and track calls may take turns.
    // Both tables wait for the last track call, whichever of them it read.
    struct Tracks {
        sd::KeptTable<sd::RecTrackDev> layout;   // [K] in `order`: the destinations
        int32_t L = 0;
        sd::KeptTable<int32_t> ls_begin;     // [K + 1] the last_seen prefix of buffer length L
        sd::DeviceBuffer last_seen;          // the scan's tables end to end: scratch the handle keeps and grows, outside the block
        sd::RecTrackDesc desc{};
        void read_on(hipStream_t stream) { layout.last = ls_begin.last = stream; }
    } tracks;

    // The level meters (syldet_recordings_levels.cpp): the reading prefix of (L, P), apart from the tracks' tables.
    struct Levels {
        int32_t L = 0;
        int64_t P = 0;
        sd::KeptTable<int64_t> first;        // reading_first [K + 1] | slot_first [K]
        sd::RecLevelsDesc desc{};
    } levels;
};

namespace sd {

// The checks the calls on a handle share, with the texts tests and the tool match on.
inline int stride_arg(const syldet_recordings *r, int64_t channel_stride)
{
    return channel_stride < r->plan.row_samples ? fail(SYLDET_ERR_INVALID_ARGUMENT, "channel_stride below row_samples") : SYLDET_OK;
}
inline int source_args(int K, const int64_t *src_offset, const int32_t *src_step)   // (NULL step: all 1)
{
    for (int k = 0; k < K; k++)
        if (src_offset[k] < 0 || (src_step && src_step[k] < 1))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "a negative source offset or a step below 1 (recording " + std::to_string(k) + ")");
    return SYLDET_OK;
}

// A source of the files' own bytes (syldet_recordings_load_pcm_device, syldet_recordings_load_sinc_pcm_device): src_offset and
// src_step count bytes, and recording k's samples are format[k] values (pcm_values.hpp).  NULL where the source is an array of
// elements (the fp32 and int16 calls): format 0 in the kept tables, so a byte source never compares equal to one of elements.
struct PcmSrc {
    int64_t bytes;
    const int32_t *format;
};
inline int format_of(const PcmSrc *pcm, int k) { return pcm ? pcm->format[k] : 0; }
inline int32_t step_of(const PcmSrc *pcm, const int32_t *src_step, int k)     // (NULL steps: contiguous recordings)
{
    return src_step ? src_step[k] : pcm ? pcm_sample_bytes(pcm->format[k]) : 1;
}

// The refusals of a byte source, behind the plain load's own checks: count(k) samples of recording k are read (none where <= 0)
template <class Count>
int pcm_args(int K, const void *d_src, const PcmSrc &pcm, const int64_t *src_offset, const int32_t *src_step, Count count)
{
    if (pcm.bytes < 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_bytes is negative");
    for (int k = 0; k < K; k++) {
        auto rec = [k]() { return " (recording " + std::to_string(k) + ")"; };
        const int64_t size = pcm_sample_bytes(pcm.format[k]), step = step_of(&pcm, src_step, k);
        if (size == 0) return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_format " + std::to_string(pcm.format[k]) + " is no sample format" + rec());
        if (step < size) return fail(SYLDET_ERR_INVALID_ARGUMENT, "src_byte_step " + std::to_string(step) + " is below the " + std::to_string(size) + " bytes of a sample" + rec());
        if (pcm.format[k] != kPcmU8 && pcm.format[k] != kPcmS24 && (((uintptr_t)d_src + (uintptr_t)src_offset[k]) % (uintptr_t)size != 0 || step % size != 0))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "an address or a step that is no multiple of the " + std::to_string(size) + " bytes of a sample" + rec());
        const int64_t n = count(k);
        // the last sample byte is offset + (n - 1) step + size - 1 < src_bytes
        if (n > 0 && (pcm.bytes < size || src_offset[k] > pcm.bytes - size || n - 1 > (pcm.bytes - size - src_offset[k]) / step))
            return fail(SYLDET_ERR_INVALID_ARGUMENT, "the samples reach beyond src_bytes" + rec());
    }
    return SYLDET_OK;
}

}  // namespace sd
