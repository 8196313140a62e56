// nearest_query.h — the pieces of a gs4d_nearest_neighbours call (include/gs4d.h) as plain C++ inline functions: the one text of the
// definition beyond what neighbour_query.h already has (the centre, takes_part, the radius check, the cells).  csrc/nearest.hip evaluates them on
// the device, host/gs4d_host.cpp (gs4d_host_nearest_neighbours) on the CPU.  float32, every product and every sum rounded on its own in the order
// the parentheses give (build without contraction).  Include it after gs4d.h (gs4d_nearest_query, GS4D_NN_*, GS4D_ID_NONE) and <math.h> / <cmath>.
#ifndef GS4D_NEAREST_QUERY_H
#define GS4D_NEAREST_QUERY_H

#include "neighbour_query.h"

namespace gs4d_nearest {

constexpr uint32_t K_MAX = 16;

// a query the device call takes: known flags, zero reserved words, 1 <= k <= 16, and the radius of gs4d_count_neighbours
GS4D_HD inline bool query_ok(const gs4d_nearest_query& q) {
    const uint32_t known = (uint32_t)(GS4D_NN_SKIP_HIDDEN | GS4D_NN_SKIP_DEAD | GS4D_NN_INCLUDE_SELF);
    return (q.flags & ~known) == 0u && q.reserved[0] == 0u && q.reserved[1] == 0u && q.reserved[2] == 0u && q.reserved[3] == 0u && q.k != 0u && q.k <= K_MAX &&
           gs4d_neighbour::radius_ok(q.radius);
}
// the stride rule of every record call, and room for the k slots
GS4D_HD inline bool stride_ok(size_t hit_stride, uint32_t k) {
    return hit_stride >= 16 && hit_stride <= 1024 && hit_stride % 16 == 0 && hit_stride >= 8 * (size_t)k;
}

// the squared distance of two centres: the three lines of gs4d_neighbour::near, restated — the very value it compares with r * r
GS4D_HD inline float dist2(const float a[3], const float b[3]) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

GS4D_HD inline uint32_t bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, sizeof u); return u; }

// The order key of candidate j at squared distance d2 (>= +0, not a NaN: its bit pattern is in float order): by distance, then by index.  The low
// word is the `record` and the high word the bits of the `dist2` of a gs4d_neighbour_hit.
GS4D_HD inline uint64_t order_key(float d2, uint32_t j) { return ((uint64_t)bits(d2) << 32) | j; }
// an empty slot, {GS4D_ID_NONE, +inf}: above the key of every candidate (dist2 <= r * r is finite)
constexpr uint64_t EMPTY = ((uint64_t)0x7F800000u << 32) | 0xFFFFFFFFull;

// `best`: K keys ascending, EMPTY behind the filled ones.  insert keeps the K smallest of what it has been given.  A key that is not below the
// worst is gone after one compare; otherwise every slot takes, from the top down, its lower neighbour (the key goes below it), the key (it goes
// here) or nothing — every index is a constant once the loop is unrolled, so the list lives in registers.
template <int K>
GS4D_HD inline void insert(uint64_t (&best)[K], uint64_t key) {
    if (!(key < best[K - 1])) return;
#pragma unroll
    for (int p = K - 1; p > 0; --p) {
        const uint64_t below = best[p - 1];
        best[p] = key < below ? below : (key < best[p] ? key : best[p]);
    }
    if (key < best[0]) best[0] = key;
}

} // namespace gs4d_nearest
#endif
