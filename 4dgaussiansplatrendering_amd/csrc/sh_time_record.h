// sh_time_record.h — the colour of a trained 4D set: spherical harmonics times a cosine series in time.  The per-record text of gs4d_shade_sh_t and
// gs4d_collapse_sh (include/gs4d.h): the weights of the time blocks, the effective row they fold a 4D row into, and the colour of a
// record from such a row — a restatement of gs4d_shade_sh's definition (its direction, basis, sum order, DC-only rule and clamp), so that
// shade_sh_t(rows) == shade_sh(collapse(rows)) bit for bit.  One text for the host and the device: csrc/shade_time.hip evaluates it on the device,
// host/gs4d_host.cpp (gs4d_host_sh_time_weights, gs4d_host_collapse_sh, gs4d_host_shade_sh_t) on the CPU; tests/sh_time_check.cpp compiles it
// stand-alone.  Every product and every sum is rounded on its own, in the order written: compile without contraction.  Plain C++17 but for hd.h.
#ifndef GS4D_SH_TIME_RECORD_H
#define GS4D_SH_TIME_RECORD_H
#include <cstdint>
#include <cmath>
#include "hd.h"

namespace gs4d_sht {

constexpr int MAX_DEGREE = 3, MAX_DEGREE_T = 2;
constexpr float INF = __builtin_huge_valf();

GS4D_HD constexpr uint32_t coeffs(int degree) { return (uint32_t)((degree + 1) * (degree + 1)); }
// words of an effective row, words and 16-byte pieces a 4D row is read by
GS4D_HD constexpr uint32_t row_words(int degree) { return 3u * coeffs(degree); }
GS4D_HD constexpr uint32_t row_words_t(int degree, int degree_t) { return row_words(degree) * (uint32_t)(degree_t + 1); }
GS4D_HD constexpr uint32_t row_pieces(int degree) { return (row_words(degree) + 3u) / 4u; }                              // 1, 3, 7, 12
GS4D_HD constexpr uint32_t row_pieces_t(int degree, int degree_t) { return (row_words_t(degree, degree_t) + 3u) / 4u; }

// why the two calls refuse their numbers, or null (the buffers are the operand list's)
inline const char* query_fault(uint64_t n, int degree, int degree_t, uint32_t reserved, uint64_t sh_stride) {
    if (n > 0xFFFFFFFFull) return "more than 2^32 - 1 records";
    if (degree < 0 || degree > MAX_DEGREE) return "q->degree must be 0, 1, 2 or 3";
    if (degree_t < 0 || degree_t > MAX_DEGREE_T) return "q->degree_t must be 0, 1 or 2";
    if (reserved != 0u) return "non-zero reserved field in q";
    if (sh_stride < 16u || sh_stride > 1024u || (sh_stride & 15u)) return "sh_stride must be a multiple of 16 from 16 to 1024";
    if (sh_stride < 4u * (uint64_t)row_words_t(degree, degree_t)) return "sh_stride holds fewer than 12 (degree + 1)^2 (degree_t + 1) bytes";
    return nullptr;
}
inline const char* dst_stride_fault(int degree, uint64_t dst_stride) {
    if (dst_stride < 16u || dst_stride > 1024u || (dst_stride & 15u)) return "dst_stride must be a multiple of 16 from 16 to 1024";
    if (dst_stride < 4u * (uint64_t)row_words(degree)) return "dst_stride holds fewer than 12 (degree + 1)^2 bytes";
    return nullptr;
}

// ---- the weights ----
// T_j = float32((-1)^j (2 pi)^(2j) / (2j)!), j = 1 .. 6: the series of cos(2 pi x) in s = x^2
constexpr float T1 = -19.739208802178716f, T2 = 64.93939402266828f, T3 = -85.45681720669371f, T4 = 60.24464137187664f, T5 = -26.426256783374388f,
                T6 = 7.903536371318465f;

// c of gs4d.h for x in [0, 0.25]: cos(2 pi x) within 1.561e-7, in [0, 1], 1 at 0 and 0 at 0.25
GS4D_HD inline float cos_quarter(float x) {
    const float s = x * x;
    float p = T6;
    p = (p * s) + T5;
    p = (p * s) + T4;
    p = (p * s) + T3;
    p = (p * s) + T2;
    p = (p * s) + T1;
    return (p * s) + 1.0f;
}

// w of gs4d.h for a finite v: cos(2 pi v) — the reduction to [0, 0.25] is exact
GS4D_HD inline float cos_turns(float v) {
    const float r = v - rintf(v);
    const float a = fabsf(r);
    const bool neg = a > 0.25f;
    const float x = neg ? 0.5f - a : a;
    const float c = cos_quarter(x);
    return neg ? -c : c;
}

GS4D_HD inline bool finite(float v) { return fabsf(v) < INF; }

// w[n - 1] of block n = 1 .. degree_t, and the mask of the blocks that take part (bit n - 1); a block that does not has w = 0 there
GS4D_HD inline uint32_t weights(int degree_t, float t, float inv_period, float mu_t, float w[2]) {
    const float u = (t - mu_t) * inv_period;
    uint32_t mask = 0u;
    w[0] = w[1] = 0.0f;
    GS4D_UNROLL
    for (int n = 1; n <= MAX_DEGREE_T; ++n) {
        if (n > degree_t) break;
        const float v = (float)n * u;
        if (finite(v)) { w[n - 1] = cos_turns(v); mask |= 1u << (n - 1); }
    }
    return mask;
}

// ---- the effective row ----
// word j of block n of a 4D row folded into e (block 0 first, then 1, then 2 — the order gs4d.h writes)
GS4D_HD inline float fold(int block, float e, float c, const float w[2], uint32_t mask) {
    if (block == 0) return c;
    return (mask >> (block - 1) & 1u) ? e + (w[block - 1] * c) : e;
}

// e[0 .. 3K - 1] from the 3 K (degree_t + 1) words of a row
GS4D_HD inline void effective_row(int degree, int degree_t, const float* row, const float w[2], uint32_t mask, float* e) {
    const uint32_t words = row_words(degree);
    for (uint32_t j = 0; j < words; ++j) {
        float v = row[j];
        for (int n = 1; n <= degree_t; ++n) v = fold(n, v, row[(uint32_t)n * words + j], w, mask);
        e[j] = v;
    }
}

// ---- the colour of a record from a row: gs4d_shade_sh's definition ----
constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;
constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_1 = -1.0925484305920792f, SH_C2_2 = 0.31539156525252005f, SH_C2_3 = -1.0925484305920792f, SH_C2_4 = 0.5462742152960396f;
constexpr float SH_C3_0 = -0.5900435899266435f, SH_C3_1 = 2.890611442640554f, SH_C3_2 = -0.4570457994644658f, SH_C3_3 = 0.3731763325901154f, SH_C3_4 = -0.4570457994644658f,
                SH_C3_5 = 1.445305721320277f, SH_C3_6 = -0.5900435899266435f;

// pm: floats 0..3 of the record (p, mu_t), sg: floats 20..23 (sig3, s44); c: the 3 K words of the row; out: r, g, b
template <int DEGREE>
GS4D_HD inline void colour(const float pm[4], const float sg[4], float t, float camx, float camy, float camz, const float* c, float out[3]) {
    constexpr uint32_t K = coeffs(DEGREE);
    const float k = (1.0f / sg[3]) * (t - pm[3]);
    const float mx = pm[0] + k * sg[0], my = pm[1] + k * sg[1], mz = pm[2] + k * sg[2];
    const float dx = mx - camx, dy = my - camy, dz = mz - camz;
    const float len2 = (dx * dx + dy * dy) + dz * dz;
    const bool directed = len2 > 0.0f && len2 < INF;
    const float inv = 1.0f / sqrtf(len2);
    const float x = dx * inv, y = dy * inv, z = dz * inv;
    float b[16];
    b[0] = SH_C0;
    if (DEGREE >= 1) { b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x; }
    if (DEGREE >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = SH_C2_0 * xy;
        b[5] = SH_C2_1 * yz;
        b[6] = SH_C2_2 * ((2.0f * zz - xx) - yy);
        b[7] = SH_C2_3 * xz;
        b[8] = SH_C2_4 * (xx - yy);
        if (DEGREE >= 3) {
            b[9] = (SH_C3_0 * y) * (3.0f * xx - yy);
            b[10] = (SH_C3_1 * xy) * z;
            b[11] = (SH_C3_2 * y) * ((4.0f * zz - xx) - yy);
            b[12] = (SH_C3_3 * z) * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
            b[13] = (SH_C3_4 * x) * ((4.0f * zz - xx) - yy);
            b[14] = (SH_C3_5 * z) * (xx - yy);
            b[15] = (SH_C3_6 * x) * (xx - 3.0f * yy);
        }
    }
    GS4D_UNROLL
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const float dc = b[0] * c[ch];
        float acc = dc;
        GS4D_UNROLL
        for (uint32_t kk = 1; kk < K; ++kk) acc = acc + b[kk] * c[3u * kk + ch];
        const float v = (directed ? acc : dc) + 0.5f;
        out[ch] = v > 0.0f ? v : 0.0f;                                                   // (a NaN gives 0)
    }
}

} // namespace gs4d_sht
#endif
