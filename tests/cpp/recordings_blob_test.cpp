// The layout of the packed-recordings handle's device block (csrc/recordings_blob.hpp: the carver and the sections
// syldet_recordings_create takes with it) on its own.  Built with -fsanitize=address,undefined by tests/test_recordings_host.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "recordings_blob.hpp"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); failures++; } } while (0)

static size_t rounded(size_t n) { return n % 16 ? n + 16 - n % 16 : n; }

// sections of these sizes, in this order: multiples of 16, one strictly behind the other without overlap, nothing for no bytes
static void carve(const std::vector<size_t> &sizes)
{
    sd::Carver c;
    size_t end = 0, sum = 0;
    for (size_t n : sizes) {
        const size_t before = c.total, at = c.take(n);
        CHECK(at % 16 == 0);
        CHECK(at == before && at >= end);                    // behind everything taken so far
        CHECK(c.total >= at + n && c.total - (at + n) < 16); // ... and the next begins behind its last byte, less than 16 further
        if (n == 0) CHECK(c.total == before);
        else CHECK(c.total > before);
        end = at + n;
        sum += rounded(n);
    }
    CHECK(c.total == sum);
}

// the handle's block for K recordings on C rows of `tiles` tiles
static void blob(size_t K, size_t C, size_t tiles)
{
    const sd::RecBlob b(K, C, tiles);
    // the nine sections in their order, with the bytes their tables hold
    const size_t at[9] = {b.table, b.events, b.row_begin, b.tile_first, b.sinc, b.track, b.ls_begin, b.n_samples, b.levels};
    const size_t sinc_slots = rounded(K * sd::RecBlob::kSinc);
    const size_t bytes[9] = {K * sd::RecBlob::kSlot, K * sd::RecBlob::kEvent, (C + 1) * 4, C * tiles * 4, sinc_slots + (K + C) * 4,
                             K * sd::RecBlob::kTrack, (K + 1) * 4, K * 8, (2 * K + 1) * 8};
    size_t end = 0, sum = 0;
    CHECK(at[0] == 0);
    for (int i = 0; i < 9; i++) {
        CHECK(at[i] % 16 == 0);
        CHECK(at[i] >= end);                                 // no overlap with the section in front
        CHECK(at[i] + bytes[i] <= b.total);                  // inside the block
        end = at[i] + bytes[i];
        sum += rounded(bytes[i]);
    }
    CHECK(b.total == sum + 16);                              // what the nine rounded sizes and the trailing 16 bytes always took
    // the two tables that lie inside a section
    CHECK(b.sinc_wg == b.sinc + sinc_slots && b.sinc_wg % 16 == 0 && b.sinc_wg + (K + C) * 4 <= b.track);
    CHECK(b.slot_first == b.levels + (K + 1) * 8 && b.slot_first + K * 8 <= b.total);
}

int main()
{
    carve({0, 1, 15, 16, 17});
    carve({17, 0, 0, 16, 1, 15, 0});
    carve({1, ((size_t)1 << 32) + 5, 0, 15, (size_t)1 << 33, 16});
    carve({});
    CHECK(sizeof(size_t) == 8);
    blob(0, 1, 0);
    blob(1, 1, 1);
    blob(9, 3, 2);
    if (failures == 0) std::printf("ok\n");
    return failures != 0;
}
