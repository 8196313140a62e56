// centre_query.h — whether one record takes part in a gs4d_count_centres query (include/gs4d.h), as a plain C++ inline function: the
// one text of the definition.  csrc/centres.hip evaluates it on the device, host/gs4d_host.cpp (gs4d_host_count_centres) on the CPU.  It restates the
// header's text operation by operation: float32, every product and every sum rounded on its own in the order the parentheses give (build without
// contraction), division correctly rounded, the two fmaf real fused operations.  Comparisons are written so that a NaN fails the test it is in and is
// not skipped by SKIP_DEAD.  Include it after gs4d.h (gs4d_centre_query, GS4D_CQ_*, GS4D_TIME_DEAD_ARG) and <math.h> / <cmath>.
#ifndef GS4D_CENTRE_QUERY_H
#define GS4D_CENTRE_QUERY_H

#include "hd.h"

namespace gs4d_centre {

// what the definition reads of a record: p = floats 0..2, mu_t = float 3, a = float 7 (read under GS4D_CQ_SKIP_HIDDEN only), sig3 = floats 20..22, s44 = float 23
struct Fields { float p[3], mu_t, a, sig3[3], s44; };

// The pieces gs4d_measure_records shares (csrc/measure_record.h).  The centre at time t, that of gs4d_shade_sh and GS4D_KEY_VIEW_Z, into m; returns dt
GS4D_HD inline float centre_at(float t, const Fields& r, float m[3]) {
    const float dt = t - r.mu_t;
    const float k = (1.0f / r.s44) * dt;
    m[0] = r.p[0] + (k * r.sig3[0]); m[1] = r.p[1] + (k * r.sig3[1]); m[2] = r.p[2] + (k * r.sig3[2]);
    return dt;
}
// the two skips: alpha not above 0; the time argument below GS4D_TIME_DEAD_ARG (a NaN is not)
GS4D_HD inline bool hidden(const Fields& r) { return !(r.a > 0.0f); }
GS4D_HD inline bool dead_at(float dt, const Fields& r) { return ((-0.5f * dt) * (1.0f / r.s44)) * dt < GS4D_TIME_DEAD_ARG; }

// hw, hh: half the width and the height of the context's image (W * 0.5f, H * 0.5f); mask: q.w * q.h bytes, rows bottom-up, or null
GS4D_HD inline bool takes_part(const gs4d_centre_query& q, float hw, float hh, const Fields& r, const uint8_t* mask) {
    const uint32_t tests = q.tests;
    float m[3];
    const float dt = centre_at(q.t, r, m);
    // skips
    if ((tests & (uint32_t)GS4D_CQ_SKIP_HIDDEN) && hidden(r)) return false;
    if ((tests & (uint32_t)GS4D_CQ_SKIP_DEAD) && dead_at(dt, r)) return false;
    // the volume
    if (tests & (uint32_t)(GS4D_CQ_BOX | GS4D_CQ_SPHERE)) {
        float v[3] = { m[0], m[1], m[2] };
        if (tests & (uint32_t)GS4D_CQ_FRAME) {
            const float* f = q.frame;
            for (int a = 0; a < 3; ++a) v[a] = (((f[a] * m[0]) + (f[3 + a] * m[1])) + (f[6 + a] * m[2])) + f[9 + a];
        }
        if (tests & (uint32_t)GS4D_CQ_BOX) {
            for (int a = 0; a < 3; ++a) if (!(q.box_lo[a] <= v[a] && v[a] <= q.box_hi[a])) return false;
        }
        if (tests & (uint32_t)GS4D_CQ_SPHERE) {
            const float dx = v[0] - q.sphere[0], dy = v[1] - q.sphere[1], dz = v[2] - q.sphere[2];
            if (!(((dx * dx) + (dy * dy)) + (dz * dz) <= q.sphere[3] * q.sphere[3])) return false;
        }
    }
    // the screen: project3d's expressions for the centre, then emit's (csrc/preprocess.hip)
    if (tests & (uint32_t)GS4D_CQ_SCREEN) {
        const float* V = q.view; const float* P = q.proj;
        const float pcx = (((V[0] * m[0]) + (V[4] * m[1])) + (V[8] * m[2])) + (V[12] * 1.0f);
        const float pcy = (((V[1] * m[0]) + (V[5] * m[1])) + (V[9] * m[2])) + (V[13] * 1.0f);
        const float pcz = (((V[2] * m[0]) + (V[6] * m[1])) + (V[10] * m[2])) + (V[14] * 1.0f);
        const float pcw = (((V[3] * m[0]) + (V[7] * m[1])) + (V[11] * m[2])) + (V[15] * 1.0f);
        const float psx = (((P[0] * pcx) + (P[4] * pcy)) + (P[8] * pcz)) + (P[12] * pcw);
        const float psy = (((P[1] * pcx) + (P[5] * pcy)) + (P[9] * pcz)) + (P[13] * pcw);
        const float psw = (((P[3] * pcx) + (P[7] * pcy)) + (P[11] * pcz)) + (P[15] * pcw);
        const float rw = 1.0f / psw;
        const float nx = rw * psx, ny = rw * psy;
        const float wx = fmaf(nx, hw, hw), wy = fmaf(ny, hh, hh);
        const float depth = -pcz;
        if (!(psw > 0.0f)) return false;
        if (!(q.depth_min <= depth && depth <= q.depth_max)) return false;
        if (!(wx >= (float)q.x && wx < (float)(q.x + q.w))) return false;
        if (!(wy >= (float)q.y && wy < (float)(q.y + q.h))) return false;
        // (the four comparisons have passed: both differences are inside the rectangle)
        if (mask && mask[(size_t)((int)floorf(wy) - q.y) * (size_t)q.w + (size_t)((int)floorf(wx) - q.x)] == 0) return false;
    }
    return true;
}

} // namespace gs4d_centre
#endif
