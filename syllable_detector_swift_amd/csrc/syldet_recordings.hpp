// syldet_recordings.hpp -- the packed-recordings handle (struct syldet_recordings) for the host files that share it:
// syldet_recordings.cpp (the plan, the loads, the events), syldet_recordings_tracks.cpp (the per-sample tracks) and
// syldet_recordings_levels.cpp (the level meters).  Not installed.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "kernels.hpp"
#include "syldet_internal.hpp"

struct syldet_recordings {
    sd::BankInfo bank{};
    int K = 0;
    std::vector<syldet_slot_t> slots;        // [K] the caller's order
    int64_t row_samples = 0, row_evals = 0;
    double fill = 0.0;
    // the load kernel's table: slots sorted by (row, offset); order[i] = the recording of table entry i
    std::vector<sd::RecSlotDev> table;
    std::vector<int32_t> order;
    std::vector<int64_t> src_offset;         // [K] the sources the device table holds (empty: none yet)
    std::vector<int32_t> src_step;
    hipStream_t last_load = nullptr;
    void *d_blob = nullptr;                  // table | events | row_begin | tile_first | the converting load's slots | its workgroup prefixes
    sd::RecLoadDesc load{};
    const sd::RecEventDev *d_events = nullptr;
    // the converting load (syldet_recordings_load_sinc_device*): its own kept sources and tables, so that plain and converting
    // loads may take turns on one handle
    std::vector<int32_t> row_begin;          // [C + 1] the table's rows
    bool sinc_kept = false;
    hipStream_t sinc_last_load = nullptr;
    std::vector<int64_t> sinc_offset, sinc_samples;   // [K]
    std::vector<int32_t> sinc_step;
    std::vector<double> sinc_rate;
    int32_t sinc_Z = 0;
    double sinc_beta = 0.0, sinc_rho = 0.0;
    std::vector<char> sinc_host;             // slots [K] | prefixes [K + C]: what one copy uploads
    size_t sinc_wg_at = 0;                   // where the prefixes begin in it (and behind d_sinc)
    char *d_sinc = nullptr;                  // (inside d_blob)
    sd::RecSincDesc sinc{};
    // the per-sample tracks (syldet_recordings_tracks.cpp): the kept destination layout and the kept buffer length, apart from
    // the loads' sources, so loads and track calls may take turns
    syldet_t *h = nullptr;                   // the bank (it outlives this handle): its thresholds and its profile
    bool track_kept = false;
    hipStream_t track_last = nullptr;        // the stream of the last track call
    std::vector<int64_t> track_offset;       // [K] the destinations the device table holds
    std::vector<int32_t> track_step;
    std::vector<sd::RecTrackDev> track_host; // [K] in the table's order: what one copy uploads
    int32_t track_L = 0;                     // the buffer length ls_begin was made for (0: none yet)
    std::vector<int32_t> ls_host;            // [K + 1]
    sd::RecTrackDev *d_track = nullptr;      // (inside d_blob)
    int32_t *d_ls_begin = nullptr;           // (inside d_blob)
    void *d_last_seen = nullptr;             // the scan's tables end to end: scratch the handle keeps and grows
    size_t last_seen_cap = 0;
    sd::RecTrackDesc track{};
    // the level meters (syldet_recordings_levels.cpp): the kept (L, P) and its reading prefix, apart from the tracks' tables
    int32_t levels_L = 0;                    // 0: none kept yet
    int64_t levels_P = 0;
    hipStream_t levels_last = nullptr;       // the stream of the last levels call
    std::vector<int64_t> levels_host;        // reading_first [K + 1] | slot_first [K]: what one copy uploads
    int64_t *d_levels_first = nullptr;       // (inside d_blob)
    sd::RecLevelsDesc levels{};
};
