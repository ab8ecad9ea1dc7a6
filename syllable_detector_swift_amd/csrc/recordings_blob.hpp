// recordings_blob.hpp -- how the packed-recordings handle (syldet_recordings.hpp) lays out its one device block.  No HIP header:
// a host program holds the arithmetic on its own (tests/cpp/recordings_blob_test.cpp).  Not installed.
#pragma once

#include <cstddef>

#include "carve.hpp"

namespace sd {

// Where every table of a handle of K recordings on C rows of `tiles` tiles begins in the block: every device pointer and every
// descriptor of the handle is the block's base plus one of these, and a new table is one more take().
struct RecBlob {
    // the bytes of kernels.hpp's RecSlotDev, RecEventDev, RecSincDev and RecTrackDev (held to them in syldet_recordings.cpp)
    static constexpr size_t kSlot = 32, kEvent = 24, kSinc = 72, kTrack = 16;
    size_t table, events, row_begin, tile_first;   // the plan: slots [K] | events [K] | row_begin [C + 1] | tile_first [C][tiles]
    size_t sinc, sinc_wg;                          // the converting load: slots [K], then (sinc_wg, inside the section) prefixes [K + C]
    size_t track, ls_begin, n_samples;             // the tracks: destinations [K] | last_seen prefix [K + 1] | lengths [K]
    size_t levels, slot_first;                     // the level meters: reading_first [K + 1], then (slot_first, right behind it) [K]
    size_t total;
    RecBlob(size_t K, size_t C, size_t tiles)
    {
        Carver c;
        table = c.take(K * kSlot);
        events = c.take(K * kEvent);
        row_begin = c.take((C + 1) * 4);
        tile_first = c.take(C * tiles * 4);
        const size_t wg_at = up16(K * kSinc);      // (the prefixes from a multiple of 16 bytes too)
        sinc = c.take(wg_at + (K + C) * 4);
        sinc_wg = sinc + wg_at;
        track = c.take(K * kTrack);
        ls_begin = c.take((K + 1) * 4);
        n_samples = c.take(K * 8);
        levels = c.take((2 * K + 1) * 8);
        slot_first = levels + (K + 1) * 8;
        total = c.total + 16;
    }
};

}  // namespace sd
