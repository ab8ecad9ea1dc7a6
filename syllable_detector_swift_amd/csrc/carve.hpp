// carve.hpp -- one device block, many tables: the rounding to 16 bytes and the carver every handle lays its block out with (the
// packed recordings' RecBlob of recordings_blob.hpp; the scorer's, the trainer's and the matchers' blocks).  No HIP header: a host
// program holds the arithmetic on its own (tests/cpp/recordings_blob_test.cpp).  Not installed.
#pragma once

#include <cstddef>

namespace sd {

// bytes (size_t) or LDS offsets (int) up to a multiple of 16
template <class T>
constexpr T up16(T n)
{
    return (n + 15) / 16 * 16;
}

// Sections taken one behind the other from one block, each from a multiple of 16 bytes; a section of no bytes takes nothing.
struct Carver {
    size_t total = 0;
    size_t take(size_t bytes)
    {
        const size_t at = total;
        total += up16(bytes);
        return at;
    }
};

}  // namespace sd
