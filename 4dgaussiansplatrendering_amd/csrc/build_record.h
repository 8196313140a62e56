// build_record.h — one 96-byte SplatData record, or its covariance alone, from splat parameters: the per-record arithmetic of gs4d_build_records
// (include/gs4d.h) as plain C++ inline functions — the one text of the definition.  csrc/build.hip evaluates them on the device,
// host/gs4d_host.cpp (gs4d_host_splat*_cov*, gs4d_host_build_records_*) on the CPU; tests/build_record_check.cpp compiles them stand-alone.  GLM 0.9.9.9's
// evaluation order is reproduced (Splat.h:91-159, 334-344): float32, every product and every sum rounded on its own in the order the parentheses give
// (build without contraction), correctly rounded division and square root.  The products are FULL products, the zeros of the scale matrices included:
// x * 0.0f is a NaN for a non-finite x and its sign decides the sign of a zero sum, so no term is left out here — the compiler drops what it can prove away.
// Matrices are column-major, element (column c, row r) = a[c * N + r].
#ifndef GS4D_BUILD_RECORD_H
#define GS4D_BUILD_RECORD_H
#include <math.h>

#include "hd.h"

namespace gs4d_build {

struct M3 { float a[9]; };
struct M4 { float a[16]; };
struct Quat { float w, x, y, z; };

// mat3 product, element = ((a0*b0) + (a1*b1)) + (a2*b2)
GS4D_HD inline M3 mm(const M3& A, const M3& B) {
    M3 R;
    GS4D_UNROLL
    for (int c = 0; c < 3; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 3; ++r) R.a[c * 3 + r] = ((A.a[r] * B.a[c * 3]) + (A.a[3 + r] * B.a[c * 3 + 1])) + (A.a[6 + r] * B.a[c * 3 + 2]);
    }
    return R;
}
GS4D_HD inline M3 tr(const M3& A) {
    M3 R;
    GS4D_UNROLL
    for (int c = 0; c < 3; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 3; ++r) R.a[c * 3 + r] = A.a[r * 3 + c];
    }
    return R;
}
// mat4 product, element = ((a0*b0 + a1*b1) + a2*b2) + a3*b3
GS4D_HD inline M4 mm(const M4& A, const M4& B) {
    M4 R;
    GS4D_UNROLL
    for (int c = 0; c < 4; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 4; ++r)
            R.a[c * 4 + r] = (((A.a[r] * B.a[c * 4]) + (A.a[4 + r] * B.a[c * 4 + 1])) + (A.a[8 + r] * B.a[c * 4 + 2])) + (A.a[12 + r] * B.a[c * 4 + 3]);
    }
    return R;
}
GS4D_HD inline M4 tr(const M4& A) {
    M4 R;
    GS4D_UNROLL
    for (int c = 0; c < 4; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 4; ++r) R.a[c * 4 + r] = A.a[r * 4 + c];
    }
    return R;
}

// rot_of: the rotation matrix of the quaternion as given (not normalised) — glm::mat3_cast
GS4D_HD inline M3 rot_of(Quat q) {
    const float xx = q.x * q.x, yy = q.y * q.y, zz = q.z * q.z, xz = q.x * q.z, xy = q.x * q.y, yz = q.y * q.z, wx = q.w * q.x, wy = q.w * q.y, wz = q.w * q.z;
    M3 R;
    R.a[0] = 1.0f - 2.0f * (yy + zz); R.a[1] = 2.0f * (xy + wz);        R.a[2] = 2.0f * (xz - wy);
    R.a[3] = 2.0f * (xy - wz);        R.a[4] = 1.0f - 2.0f * (xx + zz); R.a[5] = 2.0f * (yz + wx);
    R.a[6] = 2.0f * (xz + wy);        R.a[7] = 2.0f * (yz - wx);        R.a[8] = 1.0f - 2.0f * (xx + yy);
    return R;
}

// unit: the normalised quaternion; a length that is <= 0 gives the identity (a NaN length does not) — glm::normalize(quat)
GS4D_HD inline Quat unit(Quat q) {
    const float a = q.w * q.w, b = q.x * q.x, c = q.y * q.y, d = q.z * q.z;
    const float len = sqrtf((a + b) + (c + d));
    if (len <= 0.0f) return Quat{ 1.0f, 0.0f, 0.0f, 0.0f };
    const float inv = 1.0f / len;
    return Quat{ q.w * inv, q.x * inv, q.y * inv, q.z * inv };
}

// sigma3: ((R S) S) R^T, left to right
GS4D_HD inline M3 sigma3(Quat q, const float s[3]) {
    M3 S;
    GS4D_UNROLL
    for (int k = 0; k < 9; ++k) S.a[k] = 0.0f;
    S.a[0] = s[0]; S.a[4] = s[1]; S.a[8] = s[2];
    const M3 R = rot_of(q);
    return mm(mm(mm(R, S), S), tr(R));
}

// the covariance of a 4D splat with a velocity, Splat.h:140-158: sd = the temporal variance, td = dir * sd
GS4D_HD inline void cov_4d_vel(const float q[4], const float s[3], const float dir[3], float sd, float cov16[16]) {
    const float td[3] = { dir[0] * sd, dir[1] * sd, dir[2] * sd };
    const M3 sig = sigma3(Quat{ q[0], q[1], q[2], q[3] }, s);
    const float inv = 1.0f / sd;
    GS4D_UNROLL
    for (int c = 0; c < 3; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 3; ++r) cov16[4 * c + r] = sig.a[3 * c + r] + (td[r] * td[c]) * inv;      // sig + (1/s) * outerProduct(td, td)
        cov16[4 * c + 3] = td[c];
        cov16[12 + c] = td[c];
    }
    cov16[15] = sd;
}

// the covariance of a 4D splat with two rotations, Splat.h:91-130: (rot S) S^T rot^T with rot = L(unit q0) R(unit q1)
GS4D_HD inline void cov_4d_2q(const float q0[4], const float q1[4], const float s[4], float cov16[16]) {
    const Quat l = unit(Quat{ q0[0], q0[1], q0[2], q0[3] });
    const Quat r = unit(Quat{ q1[0], q1[1], q1[2], q1[3] });
    const M4 L = { { l.w, -l.x, -l.y, -l.z,  l.x, l.w, -l.z, l.y,  l.y, l.z, l.w, -l.x,  l.z, -l.y, l.x, l.w } };
    const M4 R = { { r.w, -r.x, -r.y, -r.z,  r.x, r.w, r.z, -r.y,  r.y, -r.z, r.w, r.x,  r.z, r.y, -r.x, r.w } };
    M4 S;
    GS4D_UNROLL
    for (int k = 0; k < 16; ++k) S.a[k] = 0.0f;
    S.a[0] = s[0]; S.a[5] = s[1]; S.a[10] = s[2]; S.a[15] = s[3];
    const M4 rot = mm(L, R);
    const M4 g = mm(mm(mm(rot, S), tr(S)), tr(rot));
    GS4D_UNROLL
    for (int k = 0; k < 16; ++k) cov16[k] = g.a[k];
}

// the mean and the colour of a 4D record
GS4D_HD inline void head_4d(const float pos[4], const float rgba[4], float o[24]) {
    o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2]; o[3] = pos[3];
    o[4] = rgba[0]; o[5] = rgba[1]; o[6] = rgba[2]; o[7] = rgba[3];
}

// GS4D_PARAMS_3D
GS4D_HD inline void record_3d(const float pos[3], const float q[4], const float s[3], const float rgba[4], float o[24]) {
    const M3 g = sigma3(Quat{ q[0], q[1], q[2], q[3] }, s);
    o[0] = pos[0]; o[1] = pos[1]; o[2] = pos[2]; o[3] = 0.0f;                            // mu_t = 0
    o[4] = rgba[0]; o[5] = rgba[1]; o[6] = rgba[2]; o[7] = rgba[3];
    GS4D_UNROLL
    for (int c = 0; c < 3; ++c) { o[8 + 4 * c] = g.a[3 * c]; o[9 + 4 * c] = g.a[3 * c + 1]; o[10 + 4 * c] = g.a[3 * c + 2]; o[11 + 4 * c] = 0.0f; }
    o[20] = 0.0f; o[21] = 0.0f; o[22] = 0.0f; o[23] = 1.0f;                              // Sigma44 = 1
}

// GS4D_PARAMS_4D_VEL, sd = the temporal variance
GS4D_HD inline void record_4d_vel(const float pos[4], const float q[4], const float s[3], const float dir[3], float sd, const float rgba[4], float o[24]) {
    head_4d(pos, rgba, o);
    cov_4d_vel(q, s, dir, sd, o + 8);
}

// GS4D_PARAMS_4D_2Q
GS4D_HD inline void record_4d_2q(const float pos[4], const float q0[4], const float q1[4], const float s[4], const float rgba[4], float o[24]) {
    head_4d(pos, rgba, o);
    cov_4d_2q(q0, q1, s, o + 8);
}

} // namespace gs4d_build
#endif
