// neighbour_query.h — the pieces of a gs4d_count_neighbours call (include/gs4d.h) as plain C++ inline functions: the one text of the
// definition.  csrc/neighbours.hip evaluates them on the device, host/gs4d_host.cpp (gs4d_host_count_neighbours) on the CPU.  They restate the
// header's text operation by operation: float32, every product and every sum rounded on its own in the order the parentheses give (build without
// contraction), division correctly rounded.  The centre and the two skips are centre_query.h's.  The cell function and the bucket hash belong to the
// device's search structure alone — the definition is the brute-force double loop over takes_part and near, and no structure may change its result —
// but they live here so that there is one text of them too (tests/neighbour_cases.py restates them for the premises of the tests).
// Include it after gs4d.h (gs4d_neighbour_query, GS4D_NB_*, GS4D_TIME_DEAD_ARG), centre_query.h and <math.h> / <cmath>.
#ifndef GS4D_NEIGHBOUR_QUERY_H
#define GS4D_NEIGHBOUR_QUERY_H

#include "centre_query.h"

namespace gs4d_neighbour {

using gs4d_centre::Fields;

// a query the device call takes: known flags, zero reserved words, cap >= 1, and 2^-63 <= r < 2^64 — r * r is then a normal float32 number
GS4D_HD inline bool radius_ok(float r) {
    const float rr = r * r;
    return r > 0.0f && r <= 3.4028234664e38f && rr <= 3.4028234664e38f && rr >= 1.17549435082e-38f;
}
GS4D_HD inline bool query_ok(const gs4d_neighbour_query& q) {
    const uint32_t known = (uint32_t)(GS4D_NB_SKIP_HIDDEN | GS4D_NB_SKIP_DEAD | GS4D_NB_COUNT_SELF);
    return (q.flags & ~known) == 0u && q.reserved[0] == 0u && q.reserved[1] == 0u && q.reserved[2] == 0u && q.reserved[3] == 0u && q.cap != 0u && radius_ok(q.radius);
}

GS4D_HD inline bool finite1(float v) { return fabsf(v) < __builtin_huge_valf(); }      // (a NaN fails the comparison)

// whether the record takes part at time t under the GS4D_NB_* flags; m: its centre (written whatever the answer)
GS4D_HD inline bool takes_part(float t, uint32_t flags, const Fields& r, float m[3]) {
    const float dt = gs4d_centre::centre_at(t, r, m);
    if ((flags & (uint32_t)GS4D_NB_SKIP_HIDDEN) && gs4d_centre::hidden(r)) return false;
    if ((flags & (uint32_t)GS4D_NB_SKIP_DEAD) && gs4d_centre::dead_at(dt, r)) return false;
    return finite1(m[0]) && finite1(m[1]) && finite1(m[2]);
}

// rr = r * r, rounded once
GS4D_HD inline bool near(const float a[3], const float b[3], float rr) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return ((dx * dx) + (dy * dy)) + (dz * dz) <= rr;
}

// ---- the search structure: cells of edge h = 2 R, R = r * (1 + 2^-10) ----
// A pair that passes `near` has |a[x] - b[x]| < R in real numbers on every axis (r * r is normal), so b[x] lies strictly between
// a[x] - R and a[x] + R, hence — float rounding is monotone, and b[x] is a float — between those two sums as float32 evaluates them; and every step
// of cell() is monotone non-decreasing in v.  cell(b[x]) therefore lies in [cell(a[x] - R), cell(a[x] + R)].
struct Grid { float R, inv_h; };
GS4D_HD inline Grid grid(float r) {
    const float R = r * 1.0009765625f;
    const float h = 2.0f * R;
    return Grid{ R, 1.0f / h };
}
constexpr float CELL_MIN = -4194304.0f, CELL_MAX = 4194303.0f;      // 23 bits of cell per axis: every value is an exact float32 and an int32
GS4D_HD inline int32_t cell(float v, float inv_h) {
    float f = floorf(v * inv_h);                  // floorf, not truncation: coordinates cross zero
    if (!(f >= CELL_MIN)) f = CELL_MIN;           // (a NaN too: no record that takes part has one)
    if (f > CELL_MAX) f = CELL_MAX;
    return (int32_t)f;
}
// the cells the ball of radius R about m can reach, per axis, both ends included
GS4D_HD inline void cell_range(const float m[3], const Grid& g, int32_t lo[3], int32_t hi[3]) {
    for (int a = 0; a < 3; ++a) { lo[a] = cell(m[a] - g.R, g.inv_h); hi[a] = cell(m[a] + g.R, g.inv_h); }
}
// the bucket of a cell: three odd multipliers, a Fibonacci mix, the top kb bits (8 <= kb <= 30).  Different cells may share a bucket.
GS4D_HD inline uint32_t bucket(int32_t cx, int32_t cy, int32_t cz, int kb) {
    const uint32_t h = ((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u) ^ ((uint32_t)cz * 83492791u);
    return (h * 2654435761u) >> (32 - kb);
}
// kb for n records: the least with 2^kb >= 2 n, inside 8 .. 30
GS4D_HD inline int bucket_bits(uint64_t n) {
    int kb = 8;
    while (kb < 30 && (1ull << kb) < 2ull * n) ++kb;
    return kb;
}
// Two different cells of one range may share a bucket; the bucket is walked for the first of them only (z outermost, x innermost), or its
// candidates would count twice.  Whether an earlier cell of the range [lo, hi] than (cx, cy, cz) has bucket b:
GS4D_HD inline bool bucket_seen(const int32_t lo[3], const int32_t hi[3], int32_t cx, int32_t cy, int32_t cz, uint32_t b, int kb) {
    for (int32_t ez = lo[2]; ez <= cz; ++ez)
        for (int32_t ey = lo[1]; ey <= (ez == cz ? cy : hi[1]); ++ey) {
            const int32_t xe = (ez == cz && ey == cy) ? cx - 1 : hi[0];
            for (int32_t ex = lo[0]; ex <= xe; ++ex) if (bucket(ex, ey, ez, kb) == b) return true;
        }
    return false;
}

} // namespace gs4d_neighbour
#endif
