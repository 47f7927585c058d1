// iiv_a2m_layout.h -- where things are in an .a2m stream: shared by the writer (iiv_a2m.hip) and the reader
// (iiv_a2m_read.hip).  include/iivision.h, sections f2 and f9.
#pragma once

#include <stddef.h>

namespace iiv {

// stream position at which tick opcode k starts: P(k) of section f9
__host__ __device__ static inline size_t tick_offset(long k)
{
    if (k < 291) return 7 + 7 * (size_t)k;
    long g = (k - 291) / 292, r = (k - 291) % 292;
    return 2048 * (size_t)(1 + g) + 7 * (size_t)r;
}

// whole 7-byte slots in a stream of `length` bytes: the k with P(k) + 7 <= length
__host__ __device__ static inline long slot_count(size_t length)
{
    if (length < 2048) return length < 14 ? 0 : (long)((length - 7) / 7 < 291 ? (length - 7) / 7 : 291);
    const size_t full = length / 2048, rem = length % 2048;
    return 291 + 292 * (long)(full - 1) + (long)(rem / 7 < 292 ? rem / 7 : 292);
}

}  // namespace iiv
