// footprint_rect.h — the pixel rectangle of a projected splat: which pixel centres the compositor has to test ("The pixel
// rectangle").  csrc/preprocess.hip evaluates it on the device in emit(); tests/footprint_rect_check.cpp compiles the same text for the CPU and
// checks, pixel by pixel, that no fragment the compositor accepts lies outside it.
//
// A fragment at the pixel offset d = (dx, dy) from the centre has the quad coordinates u = a0 . d, v = a1 . d with a0 = (e0 / s0) / (sx, sy),
// a1 = (e1 / s1) / (sx, sy): d = (sx, sy) * (e0 s0 u + e1 s1 v).  The compositor keeps it when |u| <= 0.5, |v| <= 0.5 and
// cg = 2^(-46.16624 (u^2 + v^2)) >= 0.0001, that is u^2 + v^2 <= log2(10^4) / 46.16624 = 0.287823: the quad cut by a disc of radius 0.53649.
//   the quad's box:  |dx| <= 0.5 (|e0x| s0 + |e1x| s1) |sx|               (hx of the projected record)
//   the disc's box:  |dx| <= rho sqrt((e0x s0)^2 + (e1x s1)^2) |sx|        (Cauchy-Schwarz over u^2 + v^2 <= rho^2)
// Both hold, so the smaller one does, per axis.  For an axis-aligned splat the disc's box is the wider one (0.5365 against 0.5); for one
// turned by 45 degrees with s0 = s1 it is 0.5365 / 0.7071 = 0.76 of the quad's.
//
// rho^2 = FOOT_RHO2 = 0.2885 stands 6.8e-4 above the threshold.  What that has to dominate is the rounding of q = u^2 + v^2 as the compositor
// computes it.  With U = 2^-24 and K = max(s0, s1) / min(s0, s1): a pixel whose true (u, v) lies within the disc's neighbourhood has
// |d / (sx, sy)| <= rho max(s), so each of the two products in u = fma(a0x, dx, a0y * dy) is at most rho K in magnitude; a0x carries 3 U (a
// reciprocal, a product, a quotient), dx = fx - cx 1 U, the product and the sum 1 U each, 6 U per term: |du| <= 2 * 6 U * rho K
// = 12 U rho K, the same for v, hence |dq| <= 2 (|u| |du| + |v| |dv|) <= 2 * sqrt(2) rho * 12 U rho K = 34 U rho^2 K = 5.8e-7 K (rho^2 = 0.2885)
// — below 6.8e-4 for K <= 1170.  FOOT_MAX_ANISO = 1024 keeps to that: a more anisotropic splat gets the quad's box alone.  The other
// roundings are K-free and five orders smaller: u^2 + v^2 (3 U q), the product with the constant (U), v_exp_f32 (1 ulp of cg: 1.7e-7 in the
// exponent, 4e-9 in q), and the vectors e0, e1 being orthonormal to a few U only.  The half extent itself is rounded upwards (FOOT_UP) and the
// rectangle keeps the margin 0.01 + 1e-5 hx it always had, which covers the rounding of cx, cy and of the pixel-centre arithmetic exactly as it
// does for the quad's box.
#ifndef GS4D_FOOTPRINT_RECT_H
#define GS4D_FOOTPRINT_RECT_H

#include <math.h>
#include <stdint.h>
#include "hd.h"

namespace gs4d_footprint {

constexpr float FOOT_RHO2 = 0.2885f;             // > log2(10^4) / 46.16624130844683 = 0.2878230
constexpr float FOOT_RHO = 0.53712196f;          // >= sqrt(FOOT_RHO2) = 0.537121960...
constexpr float FOOT_MAX_ANISO = 1024.0f;
constexpr float FOOT_UP = 1.0f + 0x1p-20f;       // dominates the roundings of the half extent: two squares, a sum, the square root (1 ulp on the device), two products

// the square root of a value in [1e-30, inf]: the device's v_sqrt_f32 is within 1 ulp there, which FOOT_UP covers
GS4D_HD inline float foot_sqrt(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}

// The half extents (hx, hy) of the quad's box, as the projection computed them, cut down to the disc's box where that is smaller.
// e0, e1: the quad's axes; s0, s1 > 0: their lengths; sx, sy: window scale.  Anything the bound does not cover — K > FOOT_MAX_ANISO, a
// sum of squares that underflows, a NaN — leaves the quad's extent: fminf returns its other operand for a NaN.
GS4D_HD inline void tighten(float e0x, float e0y, float e1x, float e1y, float s0, float s1, float sx, float sy, float& hx, float& hy) {
    const float lo = fminf(s0, s1), hi = fmaxf(s0, s1);
    if (!(hi <= FOOT_MAX_ANISO * lo)) return;
    const float ax = e0x * s0, bx = e1x * s1, ay = e0y * s0, by = e1y * s1;
    const float qx = ax * ax + bx * bx, qy = ay * ay + by * by;
    if (qx >= 1e-30f) hx = fminf(hx, ((FOOT_RHO * FOOT_UP) * foot_sqrt(qx)) * fabsf(sx));
    if (qy >= 1e-30f) hy = fminf(hy, ((FOOT_RHO * FOOT_UP) * foot_sqrt(qy)) * fabsf(sy));
}

// Pixel rectangle (x0 | y0 << 16, x1 | y1 << 16; (1, 0): empty) of the pixels of a W x H image whose centre lies within (hx, hy) of (cx, cy),
// grown by (mx, my).  All arguments finite.
GS4D_HD inline void pixel_rect(float cx, float cy, float hx, float hy, float mx, float my, int W, int H, uint32_t& rect0, uint32_t& rect1) {
    float fx0 = ceilf(cx - hx - mx - 0.5f), fx1 = floorf(cx + hx + mx - 0.5f);
    float fy0 = ceilf(cy - hy - my - 0.5f), fy1 = floorf(cy + hy + my - 0.5f);
    fx0 = fmaxf(fx0, 0.0f); fy0 = fmaxf(fy0, 0.0f);
    fx1 = fminf(fx1, (float)(W - 1)); fy1 = fminf(fy1, (float)(H - 1));
    rect0 = 1u; rect1 = 0u;
    if (fx0 <= fx1 && fy0 <= fy1) {
        rect0 = (uint32_t)fx0 | ((uint32_t)fy0 << 16);
        rect1 = (uint32_t)fx1 | ((uint32_t)fy1 << 16);
    }
}

} // namespace gs4d_footprint

#endif
