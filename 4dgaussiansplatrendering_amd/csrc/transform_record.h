// transform_record.h — one 96-byte SplatData record under a 4D affine map x' = L x + o: the per-record arithmetic of gs4d_transform_records
// (include/gs4d.h) as a plain C++ inline function.  csrc/transform.hip evaluates it on the device; tests/transform_record_check.cpp
// compiles the same text for the CPU, where it is compared with gs4d_host_transform_records of host/gs4d_host.cpp — the definition.  It restates the
// header's text operation by operation: float32, every product and every sum rounded on its own in the order the parentheses give (build without
// contraction).  The products are FULL products: x * 0.0f is a NaN for a non-finite x and its sign decides the sign of a zero sum, so no term is left
// out for a zero of L, all 16 elements of Sigma' are evaluated and nothing is mirrored.
// l is column-major, L[r, c] = l[4 * c + r]; the record's Sigma likewise, element (column c, row r) = float 8 + 4 * c + r; row / column 3 = time.
#ifndef GS4D_TRANSFORM_RECORD_H
#define GS4D_TRANSFORM_RECORD_H

#if defined(__HIPCC__)
#define GS4D_XF_HD __host__ __device__
#define GS4D_XF_UNROLL _Pragma("unroll")
#else
#define GS4D_XF_HD
#define GS4D_XF_UNROLL
#endif

namespace gs4d_transform {

// out (24 floats) <- the record in (24 floats) under (l[16], o[4]); in and out must not overlap
GS4D_XF_HD inline void record(const float l[16], const float o[4], const float in[24], float out[24]) {
    // the mean: L p + o
    GS4D_XF_UNROLL
    for (int r = 0; r < 4; ++r) out[r] = ((((l[r] * in[0]) + (l[4 + r] * in[1])) + (l[8 + r] * in[2])) + (l[12 + r] * in[3])) + o[r];
    // rgba
    GS4D_XF_UNROLL
    for (int k = 4; k < 8; ++k) out[k] = in[k];
    // T = L Sigma
    float T[16];
    GS4D_XF_UNROLL
    for (int c = 0; c < 4; ++c) {
        const float* S = in + 8 + 4 * c;
        GS4D_XF_UNROLL
        for (int r = 0; r < 4; ++r) T[4 * c + r] = (((l[r] * S[0]) + (l[4 + r] * S[1])) + (l[8 + r] * S[2])) + (l[12 + r] * S[3]);
    }
    // Sigma' = T L^T
    GS4D_XF_UNROLL
    for (int c = 0; c < 4; ++c) {
        GS4D_XF_UNROLL
        for (int r = 0; r < 4; ++r) out[8 + 4 * c + r] = (((T[r] * l[c]) + (T[4 + r] * l[4 + c])) + (T[8 + r] * l[8 + c])) + (T[12 + r] * l[12 + c]);
    }
}

} // namespace gs4d_transform
#endif
