// sh_rotate_record.h — one row of a spherical-harmonic table under the rotation of the map that moves its record: the per-row text of gs4d_rotate_sh
// (include/gs4d.h) as plain C++ inline functions on top of pose_record.h — the one text of the definition.  csrc/sh_rotate.hip
// evaluates it on the device, host/gs4d_host.cpp (gs4d_host_sh_rotation, gs4d_host_rotate_sh) on the CPU; tests/sh_rotate_check.cpp compiles it
// stand-alone.  It follows the header's text operation by operation: float32, every product and every sum rounded on its own in the order the
// parentheses give (build without contraction), FULL products.  Only + - * are used past the frame, which also takes 1.0f / sqrtf.  Every index below
// is a template argument or the counter of a loop with a fixed trip count: nothing is indexed by a runtime value, so on the device everything stays
// in registers.
//
// A band matrix D_L is (2L + 1) x (2L + 1), row-major; D(m, n) with m, n = -L .. L stands at D[(m + L) * (2L + 1) + (n + L)].  A row's coefficient
// c_k of channel ch is word 3k + ch; band L holds k = L^2 .. L^2 + 2L.
#ifndef GS4D_SH_ROTATE_RECORD_H
#define GS4D_SH_ROTATE_RECORD_H

#include <math.h>

#include "pose_record.h"

namespace gs4d_shrot {

constexpr int WORDS = 84;                                 // d[84]: D_1 at 0, D_2 at 9, D_3 at 34, word 83 is 0
constexpr int AT1 = 0, AT2 = 9, AT3 = 34;
constexpr int coeffs(int degree) { return (degree + 1) * (degree + 1); }

// ---- the frame ------------------------------------------------------------------------------------------------------------------------------------
GS4D_HD inline float dot3(const float a[3], const float b[3]) { return ((a[0] * b[0]) + (a[1] * b[1])) + (a[2] * b[2]); }

// e <- u * (1.0f / sqrtf(|u|^2)); false (e not written) unless the squared length is > 0 and finite
GS4D_HD inline bool unit3(const float u[3], float e[3]) {
    const float n = dot3(u, u);
    if (!(n > 0.0f) || !(n < __builtin_huge_valf())) return false;
    const float inv = 1.0f / sqrtf(n);
    GS4D_UNROLL
    for (int r = 0; r < 3; ++r) e[r] = u[r] * inv;
    return true;
}

// The Gram-Schmidt frame of the columns 0, 1, 2 of the spatial block of l (a_c[r] = l[4c + r]): e[3c + r] = component r of e_c.  False: the map
// does not rotate.
GS4D_HD inline bool frame(const float l[16], float e[9]) {
    const float* const a0 = l, * const a1 = l + 4, * const a2 = l + 8;
    float* const e0 = e, * const e1 = e + 3, * const e2 = e + 6;
    if (!unit3(a0, e0)) return false;
    const float d01 = dot3(e0, a1);
    float u1[3];
    GS4D_UNROLL
    for (int r = 0; r < 3; ++r) u1[r] = a1[r] - (d01 * e0[r]);
    if (!unit3(u1, e1)) return false;
    const float d02 = dot3(e0, a2), d12 = dot3(e1, a2);
    float u2[3];
    GS4D_UNROLL
    for (int r = 0; r < 3; ++r) u2[r] = (a2[r] - (d02 * e0[r])) - (d12 * e1[r]);
    return unit3(u2, e2);
}

// D_1 = P R P^T with R[r][c] = e_c[r] and P the signed permutation (x, y, z) -> (-y, z, -x): entry (i, j) is s_i s_j R[a_i][a_j] with
// a = (1, 2, 0), s = (-, +, -) — a move or a negation, no arithmetic
GS4D_HD inline void band1(const float e[9], float D1[9]) {
    D1[0] = e[3 * 1 + 1];  D1[1] = -e[3 * 2 + 1]; D1[2] = e[3 * 0 + 1];
    D1[3] = -e[3 * 1 + 2]; D1[4] = e[3 * 2 + 2];  D1[5] = -e[3 * 0 + 2];
    D1[6] = e[3 * 1 + 0];  D1[7] = -e[3 * 2 + 0]; D1[8] = e[3 * 0 + 0];
}

// ---- the recurrence: D_L from D_1 and D_(L-1) (Ivanic & Ruedenberg 1996, with the 1998 corrections) ---------------------------------------------------
// The coefficients by |m| (row) and |n| (column), each rounded to float32 from
//     u = sqrt((L + m)(L - m) / den)      v = (m == 0 ? -1 : 1) * sqrt((1 + [m == 0]) (L + |m| - 1)(L + |m|) / den) / 2, times sqrt 2 where |m| == 1
//     w = -sqrt((L - |m| - 1)(L - |m|) / den) / 2
// with den = (L + n)(L - n) for |n| < L and 2L (2L - 1) for |n| == L.  A zero stands where the term is left out (u: |m| == L; w: m == 0 or |m| >= L - 1).
template <int L> GS4D_HD constexpr float coef_u(int am, int an);
template <int L> GS4D_HD constexpr float coef_v(int am, int an);
template <int L> GS4D_HD constexpr float coef_w(int am, int an);
template <> GS4D_HD constexpr float coef_u<2>(int am, int an) {
    constexpr float t[3][3] = { { 1.0f, 1.1547005383792515f, 0.57735026918962573f },
                                { 0.8660254037844386f, 1.0f, 0.5f },
                                { 0.0f, 0.0f, 0.0f } };
    return t[am][an];
}
template <> GS4D_HD constexpr float coef_v<2>(int am, int an) {
    constexpr float t[3][3] = { { -0.5f, -0.57735026918962573f, -0.28867513459481287f },
                                { 0.8660254037844386f, 1.0f, 0.5f },
                                { 0.8660254037844386f, 1.0f, 0.5f } };
    return t[am][an];
}
template <> GS4D_HD constexpr float coef_w<2>(int, int) { return 0.0f; }
template <> GS4D_HD constexpr float coef_u<3>(int am, int an) {
    constexpr float t[4][4] = { { 1.0f, 1.0606601717798212f, 1.3416407864998738f, 0.54772255750516607f },
                                { 0.94280904158206336f, 1.0f, 1.2649110640673518f, 0.5163977794943222f },
                                { 0.7453559924999299f, 0.79056941504209488f, 1.0f, 0.40824829046386302f },
                                { 0.0f, 0.0f, 0.0f, 0.0f } };
    return t[am][an];
}
template <> GS4D_HD constexpr float coef_v<3>(int am, int an) {
    constexpr float t[4][4] = { { -0.57735026918962573f, -0.61237243569579447f, -0.7745966692414834f, -0.31622776601683794f },
                                { 0.81649658092772603f, 0.8660254037844386f, 1.0954451150103321f, 0.44721359549995793f },
                                { 0.7453559924999299f, 0.79056941504209488f, 1.0f, 0.40824829046386302f },
                                { 0.9128709291752769f, 0.96824583655185426f, 1.2247448713915889f, 0.5f } };
    return t[am][an];
}
template <> GS4D_HD constexpr float coef_w<3>(int am, int an) {
    constexpr float t[4] = { -0.23570226039551584f, -0.25f, -0.31622776601683794f, -0.12909944487358055f };
    return am == 1 ? t[an] : 0.0f;
}

constexpr int iabs(int a) { return a < 0 ? -a : a; }

// P(i, a, n) of band L: one or two products of an element of D_1 (row i) and an element of D_(L-1) (row a)
template <int L, int I, int A, int N>
GS4D_HD inline float P(const float* D1, const float* Dp) {
    constexpr int WP = 2 * L - 1, E = L - 1;                                        // D_(L-1): its width, its last column
    const float* const r1 = D1 + (I + 1) * 3 + 1;                                   // r1[j] = D_1(i, j)
    const float* const rp = Dp + (A + E) * WP + E;                                  // rp[b] = D_(L-1)(a, b)
    if (N == L) return (r1[1] * rp[E]) - (r1[-1] * rp[-E]);
    if (N == -L) return (r1[1] * rp[-E]) + (r1[-1] * rp[E]);
    return r1[0] * rp[N == L || N == -L ? 0 : N];
}

// D_L(m, n) = ((u * U) + (v * V)) + (w * W), a term whose coefficient is a zero of the table left out
template <int L, int M, int N>
GS4D_HD inline float entry(const float* D1, const float* Dp) {
    constexpr int AM = iabs(M), AN = iabs(N);
    constexpr float u = coef_u<L>(AM, AN), v = coef_v<L>(AM, AN), w = coef_w<L>(AM, AN);
    float V;
    if (M == 0) V = P<L, 1, 1, N>(D1, Dp) + P<L, -1, -1, N>(D1, Dp);
    else if (M == 1) V = P<L, 1, 0, N>(D1, Dp);
    else if (M == -1) V = P<L, -1, 0, N>(D1, Dp);
    else if (M > 1) V = P<L, 1, (M > 1 ? M - 1 : 0), N>(D1, Dp) - P<L, -1, (M > 1 ? 1 - M : 0), N>(D1, Dp);
    else V = P<L, 1, (M < -1 ? M + 1 : 0), N>(D1, Dp) + P<L, -1, (M < -1 ? -M - 1 : 0), N>(D1, Dp);
    float acc = v * V;
    if (AM < L) acc = (u * P<L, 0, (AM < L ? M : 0), N>(D1, Dp)) + acc;
    if (M != 0 && AM < L - 1) {
        constexpr int UP = AM < L - 1 ? AM + 1 : 0;                                  // (|m| + 1 <= L - 1: a row of D_(L-1))
        const float W = M > 0 ? P<L, 1, UP, N>(D1, Dp) + P<L, -1, -UP, N>(D1, Dp) : P<L, 1, -UP, N>(D1, Dp) - P<L, -1, UP, N>(D1, Dp);
        acc = acc + (w * W);
    }
    return acc;
}

// the entries (M, N), (M, N + 1), ... row by row to the last one
template <int L, int M, int N, bool PAST = (M > L)> struct Fill {
    static GS4D_HD inline void run(const float* D1, const float* Dp, float* D) {
        D[(M + L) * (2 * L + 1) + (N + L)] = entry<L, M, N>(D1, Dp);
        Fill<L, (N == L ? M + 1 : M), (N == L ? -L : N + 1)>::run(D1, Dp, D);
    }
};
template <int L, int M, int N> struct Fill<L, M, N, true> { static GS4D_HD inline void run(const float*, const float*, float*) {} };

// D <- D_L, L = 2 (Dp = D1) or 3 (Dp = D_2); D must not overlap D1 or Dp
template <int L>
GS4D_HD inline void band(const float* D1, const float* Dp, float* D) { Fill<L, -L, -L>::run(D1, Dp, D); }

// ---- the application -----------------------------------------------------------------------------------------------------------------------------
// band L of the row's coefficient words c, in place: per channel and output coefficient i, acc = D[i][0]*c_0, then acc = acc + (D[i][j]*c_j) in ascending j
template <int L>
GS4D_HD inline void apply(const float* D, float* c) {
    constexpr int W = 2 * L + 1, K0 = L * L;
    GS4D_UNROLL
    for (int ch = 0; ch < 3; ++ch) {
        float in[W];
        GS4D_UNROLL
        for (int j = 0; j < W; ++j) in[j] = c[3 * (K0 + j) + ch];
        GS4D_UNROLL
        for (int i = 0; i < W; ++i) {
            float acc = D[i * W] * in[0];
            GS4D_UNROLL
            for (int j = 1; j < W; ++j) acc = acc + (D[i * W + j] * in[j]);
            c[3 * (K0 + i) + ch] = acc;
        }
    }
}

// d[84] of the map l; false (d not written): the map does not rotate.  Bands above MAXBAND are not computed (their words are not written).
template <int MAXBAND = 3>
GS4D_HD inline bool rotation(const float l[16], float* d) {
    float e[9];
    if (!frame(l, e)) return false;
    band1(e, d + AT1);
    if (MAXBAND >= 2) band<2>(d + AT1, d + AT1, d + AT2);
    if (MAXBAND >= 3) { band<3>(d + AT1, d + AT2, d + AT3); d[WORDS - 1] = 0.0f; }
    return true;
}

// The first 3 (DEGREE + 1)^2 words of a row, in place, under the map l: words 0..2 stay.  False: the map does not rotate, nothing is written.
// D_3 is built after bands 1 and 2 are done with.
template <int DEGREE>
GS4D_HD inline bool coefficients(const float l[16], float* c) {
    if (DEGREE == 0) return true;
    float e[9], D1[9];
    if (!frame(l, e)) return false;
    band1(e, D1);
    apply<1>(D1, c);
    if (DEGREE >= 2) {
        float D2[25];
        band<2>(D1, D1, D2);
        apply<2>(D2, c);
        if (DEGREE >= 3) {
            float D3[49];
            band<3>(D1, D2, D3);
            apply<3>(D3, c);
        }
    }
    return true;
}

// ---- the map of a row -----------------------------------------------------------------------------------------------------------------------------
// GS4D_POSE_INDEX: a <- row j of the table; false for j >= m (a not written)
template <class Rows>
GS4D_HD inline bool index_map(const Rows& rows, unsigned int m, unsigned int j, float a[20]) {
    if (j >= m) return false;
    rows(j, a);
    return true;
}
// GS4D_POSE_BLEND4 is gs4d_pose::blend4 as it is

} // namespace gs4d_shrot
#endif
