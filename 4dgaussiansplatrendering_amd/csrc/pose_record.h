// pose_record.h — one 96-byte SplatData record under the map its bind row chooses among the m rows of a table: the per-record text of
// gs4d_pose_records (include/gs4d.h) as plain C++ inline functions on top of transform_record.h — the one text of the definition.
// csrc/pose.hip evaluates it on the device, host/gs4d_host.cpp (gs4d_host_pose_records) on the CPU; tests/pose_record_check.cpp compiles it
// stand-alone.  It follows the header's text operation by operation: float32, every product and every sum rounded on its own in the order the
// parentheses give (build without contraction), FULL products — a weight of 0 is multiplied like any other, so a NaN row under weight 0 gives NaN.
// `rows` is whatever fetches a row of the table: rows(j, r) fills r[20] with l[16], o[4] of row j; it is called for j < m only.
#ifndef GS4D_POSE_RECORD_H
#define GS4D_POSE_RECORD_H

#include "transform_record.h"

namespace gs4d_pose {

// out <- in, the 24 words as they are (a float move keeps the bits of a NaN)
GS4D_HD inline void copy(const float in[24], float out[24]) {
    GS4D_UNROLL
    for (int k = 0; k < 24; ++k) out[k] = in[k];
}

// GS4D_POSE_INDEX: row j of the table, or the record as it is for j >= m; in and out must not overlap
template <class Rows>
GS4D_HD inline void index(const Rows& rows, unsigned int m, unsigned int j, const float in[24], float out[24]) {
    if (j >= m) { copy(in, out); return; }
    float a[20];
    rows(j, a);
    gs4d_transform::record(a, a + 16, in, out);
}

// The blended row of GS4D_POSE_BLEND4: slot k takes part iff j[k] < m, whatever w[k] is; the first such slot gives a[e] = w[k] * row[e], every
// later one a[e] = a[e] + (w[k] * row[e]), e = 0..19.  False: no slot takes part (a is not written).
template <class Rows>
GS4D_HD inline bool blend4(const Rows& rows, unsigned int m, const unsigned int j[4], const float w[4], float a[20]) {
    bool any = false;
    GS4D_UNROLL
    for (int k = 0; k < 4; ++k) {
        if (j[k] >= m) continue;
        float r[20];
        rows(j[k], r);
        if (!any) {
            GS4D_UNROLL
            for (int e = 0; e < 20; ++e) a[e] = w[k] * r[e];
        } else {
            GS4D_UNROLL
            for (int e = 0; e < 20; ++e) a[e] = a[e] + (w[k] * r[e]);
        }
        any = true;
    }
    return any;
}

// GS4D_POSE_BLEND4: the record under the blended row, or as it is when no slot takes part; in and out must not overlap
template <class Rows>
GS4D_HD inline void blend(const Rows& rows, unsigned int m, const unsigned int j[4], const float w[4], const float in[24], float out[24]) {
    float a[20];
    if (!blend4(rows, m, j, w, a)) { copy(in, out); return; }
    gs4d_transform::record(a, a + 16, in, out);
}

} // namespace gs4d_pose
#endif
