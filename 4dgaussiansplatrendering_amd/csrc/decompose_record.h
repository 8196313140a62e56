// decompose_record.h — the splat parameters of one 96-byte record: position, colour, velocity and temporal variance, and the rotation and scales
// whose covariance the record holds — the per-record arithmetic of gs4d_decompose_records (include/gs4d.h), the inverse of
// build_record.h, as plain C++ inline functions: the one text of the definition.  csrc/decompose.hip evaluates it on the device, host/gs4d_host.cpp
// (gs4d_host_decompose_records) on the CPU; tests/decompose_record_check.cpp compiles it stand-alone.  Everything is float32, every product and
// every sum rounded on its own in the order the parentheses give (build without contraction), with correctly rounded division and square root; only
// + - * / and sqrtf are used, the rest is comparisons and selects.  Every loop has a fixed trip count and nothing is indexed by a runtime value:
// a NaN, an Inf or an indefinite matrix gives whatever this arithmetic gives.
// Matrices are column-major as in build_record.h, element (column c, row r) = a[c * N + r]; of the record's covariance the LOWER triangle is read
// (floats 8, 9, 10, 13, 14, 18: rows >= columns), the upper one is ignored.
#ifndef GS4D_DECOMPOSE_RECORD_H
#define GS4D_DECOMPOSE_RECORD_H
#include <math.h>

#include "build_record.h"
#include "hd.h"

namespace gs4d_decompose {

// Sweeps of the cyclic Jacobi: the smallest count at which the worst round-trip error over the sets of tests/decompose_cases.py stops falling
// (tools/decompose_sweeps.py; DESIGN.md §4 has the figures)
constexpr int SWEEPS = 3;

// the lower triangle of a symmetric 3x3, a_rc = element (row r, column c)
struct Sym3 { float a00, a11, a22, a10, a20, a21; };
struct Splat { float pos[4], q[4], s[3], rgba[4], dir[3], tvar; };      // what a record decomposes into; q is w x y z

GS4D_HD inline float absf(float x) { return x < 0.0f ? -x : x; }

// One Jacobi rotation in the plane (p, q), r the third axis: app, aqq the two diagonal elements, apq the element to annihilate, arp, arq the other
// two; vp, vq columns p and q of V.  Skipped — nothing changes — when apq changes neither diagonal element in float32: |app| + |apq| == |app| and
// |aqq| + |apq| == |aqq| (apq == 0 among them; a NaN anywhere is not skipped).  tau = (aqq - app) / (2 apq), t = sign(tau) / (|tau| + sqrt(1 +
// tau^2)) with sign(0) = +1, c = 1 / sqrt(1 + t^2), s = t c: an overflowing tau^2 ends in t = +-0, c = 1, s = +-0.
GS4D_HD inline void rotate(float& app, float& aqq, float& apq, float& arp, float& arq, float* vp, float* vq) {
    const float g = absf(apq);
    if (absf(app) + g == absf(app) && absf(aqq) + g == absf(aqq)) return;
    const float tau = (aqq - app) / (2.0f * apq);
    const float den = absf(tau) + sqrtf(1.0f + tau * tau);
    const float t = (tau < 0.0f ? -1.0f : 1.0f) / den;
    const float c = 1.0f / sqrtf(1.0f + t * t), s = t * c;
    const float h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0f;
    const float rp = arp, rq = arq;
    arp = (c * rp) - (s * rq);
    arq = (s * rp) + (c * rq);
    GS4D_UNROLL
    for (int k = 0; k < 3; ++k) {
        const float kp = vp[k], kq = vq[k];
        vp[k] = (c * kp) - (s * kq);
        vq[k] = (s * kp) + (c * kq);
    }
}

// compare-exchange of two (eigenvalue, column) pairs: the larger eigenvalue first; equal ones (and a NaN on either side) stay as they are
GS4D_HD inline void order(float& la, float& lb, float* va, float* vb) {
    const bool swap = lb > la;
    const float l = la;
    la = swap ? lb : la;
    lb = swap ? l : lb;
    GS4D_UNROLL
    for (int k = 0; k < 3; ++k) {
        const float x = va[k];
        va[k] = swap ? vb[k] : va[k];
        vb[k] = swap ? x : vb[k];
    }
}

// eigen3: SWEEPS sweeps of the cyclic Jacobi over the pairs (0,1), (0,2), (1,2); the eigenvalues in descending order (a stable network: ties keep
// the lower original axis first) with their columns in V; the third column is then replaced by the cross product of the first two, so V is a
// proper rotation as far as its first two columns are orthonormal
template <int N = SWEEPS>
GS4D_HD inline void eigen3(Sym3 A, float lam[3], gs4d_build::M3& V) {
    GS4D_UNROLL
    for (int k = 0; k < 9; ++k) V.a[k] = 0.0f;
    V.a[0] = 1.0f; V.a[4] = 1.0f; V.a[8] = 1.0f;
    GS4D_UNROLL
    for (int sweep = 0; sweep < N; ++sweep) {
        rotate(A.a00, A.a11, A.a10, A.a20, A.a21, V.a + 0, V.a + 3);
        rotate(A.a00, A.a22, A.a20, A.a10, A.a21, V.a + 0, V.a + 6);
        rotate(A.a11, A.a22, A.a21, A.a10, A.a20, V.a + 3, V.a + 6);
    }
    lam[0] = A.a00; lam[1] = A.a11; lam[2] = A.a22;
    order(lam[0], lam[1], V.a + 0, V.a + 3);
    order(lam[1], lam[2], V.a + 3, V.a + 6);
    order(lam[0], lam[1], V.a + 0, V.a + 3);
    V.a[6] = (V.a[1] * V.a[5]) - (V.a[2] * V.a[4]);
    V.a[7] = (V.a[2] * V.a[3]) - (V.a[0] * V.a[5]);
    V.a[8] = (V.a[0] * V.a[4]) - (V.a[1] * V.a[3]);
}

// quat_of: the unit quaternion of a rotation matrix by the largest of the four traces 4w^2, 4x^2, 4y^2, 4z^2 (Shepperd; the first of equal ones in
// the order w, x, y, z, a NaN trace falls through to z): that row of 4 q q^T, normalised by gs4d_build::unit.  Then the one of q, -q with w >= 0;
// with w == 0 (+0 or -0, which stays as it is) the one whose first non-zero of x, y, z is positive.
GS4D_HD inline gs4d_build::Quat quat_of(const gs4d_build::M3& R) {
    const float m00 = R.a[0], m10 = R.a[1], m20 = R.a[2], m01 = R.a[3], m11 = R.a[4], m21 = R.a[5], m02 = R.a[6], m12 = R.a[7], m22 = R.a[8];
    const float tw = ((1.0f + m00) + m11) + m22, tx = ((1.0f + m00) - m11) - m22, ty = ((1.0f - m00) + m11) - m22, tz = ((1.0f - m00) - m11) + m22;
    gs4d_build::Quat q;
    if (tw >= tx && tw >= ty && tw >= tz) q = gs4d_build::Quat{ tw, m21 - m12, m02 - m20, m10 - m01 };
    else if (tx >= ty && tx >= tz)        q = gs4d_build::Quat{ m21 - m12, tx, m10 + m01, m02 + m20 };
    else if (ty >= tz)                    q = gs4d_build::Quat{ m02 - m20, m10 + m01, ty, m21 + m12 };
    else                                  q = gs4d_build::Quat{ m10 - m01, m02 + m20, m21 + m12, tz };
    q = gs4d_build::unit(q);
    const bool flip = q.w < 0.0f || (q.w == 0.0f && (q.x < 0.0f || (q.x == 0.0f && (q.y < 0.0f || (q.y == 0.0f && q.z < 0.0f)))));
    return flip ? gs4d_build::Quat{ -q.w, -q.x, -q.y, -q.z } : q;
}

// rot_scale: Sigma3 -> (q, s) with Sigma3 ~ ((R S) S) R^T, R = rot_of(q): s the standard deviations in descending order, +0 for an eigenvalue
// that is negative or a zero of either sign (a NaN stays a NaN)
template <int N = SWEEPS>
GS4D_HD inline void rot_scale(const Sym3& A, float q[4], float s[3]) {
    float lam[3];
    gs4d_build::M3 V;
    eigen3<N>(A, lam, V);
    GS4D_UNROLL
    for (int k = 0; k < 3; ++k) s[k] = lam[k] <= 0.0f ? 0.0f : sqrtf(lam[k]);
    const gs4d_build::Quat u = quat_of(V);
    q[0] = u.w; q[1] = u.x; q[2] = u.y; q[3] = u.z;
}

// record: the parameters of the record `in` in the form FORM (GS4D_PARAMS_3D = 0, GS4D_PARAMS_4D_VEL = 1).  3D: pos[3], dir and tvar are not
// written, mu_t, the time row and column and Sigma44 are not looked at.  4D_VEL: tvar = Sigma44, td = floats 20..22, dir = td / tvar, Sigma3 =
// the spatial block - (td_r * td_c) * (1 / tvar): the builder's own terms, subtracted.  SOLVE == false leaves q and s unwritten.
template <int FORM, bool SOLVE, int N = SWEEPS>
GS4D_HD inline void record(const float in[24], Splat& o) {
    o.pos[0] = in[0]; o.pos[1] = in[1]; o.pos[2] = in[2];
    GS4D_UNROLL
    for (int k = 0; k < 4; ++k) o.rgba[k] = in[4 + k];
    Sym3 A = { in[8], in[13], in[18], in[9], in[10], in[14] };
    if (FORM != 0) {
        const float sd = in[23], td[3] = { in[20], in[21], in[22] };
        o.pos[3] = in[3];
        o.tvar = sd;
        GS4D_UNROLL
        for (int k = 0; k < 3; ++k) o.dir[k] = td[k] / sd;
        if (SOLVE) {
            const float inv = 1.0f / sd;
            A.a00 = A.a00 - (td[0] * td[0]) * inv; A.a11 = A.a11 - (td[1] * td[1]) * inv; A.a22 = A.a22 - (td[2] * td[2]) * inv;
            A.a10 = A.a10 - (td[1] * td[0]) * inv; A.a20 = A.a20 - (td[2] * td[0]) * inv; A.a21 = A.a21 - (td[2] * td[1]) * inv;
        }
    }
    if (SOLVE) rot_scale<N>(A, o.q, o.s);
}

} // namespace gs4d_decompose
#endif
