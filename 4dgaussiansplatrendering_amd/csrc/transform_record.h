// transform_record.h — one 96-byte SplatData record under a 4D affine map x' = L x + o: the per-record arithmetic of gs4d_transform_records
// (include/gs4d.h) as plain C++ inline functions — the one text of the definition.  csrc/transform.hip and csrc/transform_selected.hip
// evaluate it on the device, host/gs4d_host.cpp (gs4d_host_transform_records, gs4d_host_transform_selected, gs4d_host_measure_centre) on the CPU;
// tests/transform_record_check.cpp and tests/transform_selected_check.cpp compile it stand-alone.  It follows the header's text operation by operation:
// float32, every product and every sum rounded on its own in the order the parentheses give (build without contraction).  The products are FULL
// products: x * 0.0f is a NaN for a non-finite x and its sign decides the sign of a zero sum, so no term is left out for a zero of L, all 16 elements
// of Sigma' are evaluated and nothing is mirrored.
// l is column-major, L[r, c] = l[4 * c + r]; the record's Sigma likewise, element (column c, row r) = float 8 + 4 * c + r; row / column 3 = time.
#ifndef GS4D_TRANSFORM_RECORD_H
#define GS4D_TRANSFORM_RECORD_H

#include "hd.h"

namespace gs4d_transform {

// floats 8..23 of out <- L Sigma L^T of the record in (24 floats): the T and Sigma' lines of the definition (gs4d_warp_records takes them with the
// L of its lattice: warp_record.h); in and out must not overlap
GS4D_HD inline void sigma(const float l[16], const float in[24], float out[24]) {
    // T = L Sigma
    float T[16];
    GS4D_UNROLL
    for (int c = 0; c < 4; ++c) {
        const float* S = in + 8 + 4 * c;
        GS4D_UNROLL
        for (int r = 0; r < 4; ++r) T[4 * c + r] = (((l[r] * S[0]) + (l[4 + r] * S[1])) + (l[8 + r] * S[2])) + (l[12 + r] * S[3]);
    }
    // Sigma' = T L^T
    GS4D_UNROLL
    for (int c = 0; c < 4; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 4; ++r) out[8 + 4 * c + r] = (((T[r] * l[c]) + (T[4 + r] * l[4 + c])) + (T[8 + r] * l[8 + c])) + (T[12 + r] * l[12 + c]);
    }
}

// out (24 floats) <- the record in (24 floats) under (l[16], o[4]); in and out must not overlap
GS4D_HD inline void record(const float l[16], const float o[4], const float in[24], float out[24]) {
    // the mean: L p + o
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) out[r] = ((((l[r] * in[0]) + (l[4 + r] * in[1])) + (l[8 + r] * in[2])) + (l[12 + r] * in[3])) + o[r];
    // rgba
    GS4D_UNROLL
    for (int k = 4; k < 8; ++k) out[k] = in[k];
    sigma(l, in, out);
}

// gs4d_transform_selected (include/gs4d.h): out (24 floats) <- the record in (24 floats) under (l[16], o[4]) about the pivot c[3];
// in and out must not overlap.  Without a pivot it is record().  With one the spatial mean goes through record() as p - c and c is added to
// what comes out, both always, also for c == 0 (a -0 coordinate may become +0); mu_t, rgba and Sigma do not see the pivot.
GS4D_HD inline void record_about(const float l[16], const float o[4], bool pivot, const float c[3], const float in[24], float out[24]) {
    if (!pivot) { record(l, o, in, out); return; }
    float q[24];
    GS4D_UNROLL
    for (int a = 0; a < 3; ++a) q[a] = in[a] - c[a];
    GS4D_UNROLL
    for (int k = 3; k < 24; ++k) q[k] = in[k];
    record(l, o, q, out);
    GS4D_UNROLL
    for (int r = 0; r < 3; ++r) out[r] = out[r] + c[r];
}

// The centre of a measurement (the fields of a gs4d_measure), what gs4d_host_measure_centre returns — per axis, in double
// precision, lo + (hi - lo) * (cell_sum / (count * 2^20)), rounded to float; count == 0: (0, 0, 0).  Every operation is rounded on its own (build
// without contraction); double add, multiply, divide and the conversion from a 64-bit integer are correctly rounded on the device as on the host, so
// the bits are the host's.  The fields are data: non-finite ends and a huge cell_sum give what the line gives.
GS4D_HD inline void measure_centre(unsigned int count, const float lo[3], const float hi[3], const unsigned long long cell_sum[3], float c[3]) {
    GS4D_UNROLL
    for (int a = 0; a < 3; ++a) {
        if (count == 0u) { c[a] = 0.0f; continue; }
        const double l = lo[a], h = hi[a];
        const double span = h - l;
        const double cells = (double)count * 1048576.0;
        const double frac = (double)cell_sum[a] / cells;
        const double step = span * frac;
        c[a] = (float)(l + step);
    }
}

} // namespace gs4d_transform
#endif
