// lod_query.h — the predicates of gs4d_lod_cut (include/gs4d.h) as plain C++ inline functions: the one text of the definition.
// csrc/lod.hip evaluates it on the device, host/gs4d_host.cpp (gs4d_host_lod_cut) and tests/lod_query_check.cpp on the CPU.  It restates the header's
// text operation by operation: float32, every product and every sum rounded on its own in the order the parentheses give (build without
// contraction), no square root.  Comparisons are written so that a NaN distance counts as near and a NaN on either side of the last comparison is
// not fine.  Include it after gs4d.h (gs4d_lod_query) and <math.h> / <cmath>.
#ifndef GS4D_LOD_QUERY_H
#define GS4D_LOD_QUERY_H

#include "hd.h"
#include "centre_query.h"

namespace gs4d_lod {

// the state of a node: the byte of the state plane
enum : uint8_t { STOP = 0, DESCEND = 1, DRAW = 2 };

// what the predicate takes from the query, computed once: r2 = ratio * ratio, n2 = near_dist * near_dist
struct View { float eye[3], t, r2, n2; };
GS4D_HD inline View view_of(const gs4d_lod_query& q) { return View{ { q.eye[0], q.eye[1], q.eye[2] }, q.t, q.ratio * q.ratio, q.near_dist * q.near_dist }; }

// r: the fields centre_at reads (r.a is not looked at); sxx, syy, szz: floats 8, 13 and 18 of the record, the rest variances
GS4D_HD inline bool fine(const View& w, const gs4d_centre::Fields& r, float sxx, float syy, float szz) {
    float m[3];
    (void)gs4d_centre::centre_at(w.t, r, m);
    const float dx = m[0] - w.eye[0], dy = m[1] - w.eye[1], dz = m[2] - w.eye[2];
    const float dist2 = ((dx * dx) + (dy * dy)) + (dz * dz);
    const float e = dist2 > w.n2 ? dist2 : w.n2;
    float v = sxx;
    if (syy > v) v = syy;
    if (szz > v) v = szz;
    return v <= w.r2 * e;
}
// ... of the 24 floats of a record
GS4D_HD inline bool fine(const View& w, const float* p) {
    const gs4d_centre::Fields r{ { p[0], p[1], p[2] }, p[3], 0.0f, { p[20], p[21], p[22] }, p[23] };
    return fine(w, r, p[8], p[13], p[18]);
}

// a node of level k whose parent word is p: a child iff the word names a node of a higher level (next_first = level_first[k + 1]), else a root
GS4D_HD inline bool is_child(uint32_t p, uint32_t next_first, uint32_t n) { return next_first <= p && p < n; }

// the state of a node that is tested
GS4D_HD inline uint8_t tested_state(bool leaf, bool is_fine) { return leaf || is_fine ? DRAW : DESCEND; }

// whether the device call takes the query for a forest of n nodes
GS4D_HD inline bool query_ok(const gs4d_lod_query& q, uint64_t n) {
    if (n > 0xFFFFFFFEull) return false;
    if (q.levels < 1u || q.levels > 16u || q.flags != 0u) return false;
    if (q.reserved[0] != 0u || q.reserved[1] != 0u || q.reserved[2] != 0u) return false;
    if (!(q.ratio >= 0.0f)) return false;                                               // (a NaN fails)
    if (!(q.near_dist >= 0.0f && q.near_dist <= 3.402823466e+38f)) return false;      // finite
    if (q.level_first[0] != 0u || (uint64_t)q.level_first[q.levels] != n) return false;
    for (uint32_t k = 0; k < q.levels; ++k) if (q.level_first[k] > q.level_first[k + 1u]) return false;
    return true;
}

} // namespace gs4d_lod
#endif
