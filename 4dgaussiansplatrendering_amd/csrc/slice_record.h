// slice_record.h — one 96-byte SplatData record baked at one time: the per-record arithmetic of gs4d_slice_records (include/gs4d.h)
// as a plain C++ inline function — the one text of the definition.  csrc/slice.hip evaluates it on the device, host/gs4d_host.cpp
// (gs4d_host_slice_records) on the CPU.  It is the time conditioning of project_4d
// (csrc/preprocess.hip) restated operation by operation, not moved out of it: float32, every product and every difference rounded on its own in the
// order the parentheses give (build without contraction), correctly rounded division, full products (inf * 0 is a NaN).  expf is the C library's
// on the CPU and the device library's under hipcc — the call project_4d makes, so word 7 of a device slice is the alpha the device's draw computes.
// The record's Sigma: element (column c, row r) = float 8 + 4 * c + r; row / column 3 = time.
//
// Why the time row and the time column of the slice are -0 and not +0 — a draw of the slice at uTime == mu_t_out is a fixed point:
//     dt' = mu_t_out - mu_t_out = +0 (mu_t_out is finite), so k' = inv' * (+0) = +0 for every s44_out > 0, +inf included (inv' = +0);
//     k' * (-0) = -0, and x + (-0) = x for EVERY x, x = -0 included (x + (+0) would turn a -0 coordinate into +0);
//     tv'[c] = inv' * (-0) = -0, a'[r] * tv'[c] = (-0) * (-0) = +0, and x - (+0) = x for every x, -0 included (x - (-0) would turn a -0 element into +0);
//     ((-0.5f * (+0)) * inv') * (+0) = -0, expf(-0) = 1, maxf(1, min_opacity) = 1 for min_opacity <= 1, and 1 * alpha = alpha.
// So the draw's conditional centre, conditional covariance and alpha are the slice's words 0..2, 8 + 4c + r and 7 bit for bit.  The two depth-key
// expressions of depth_key.h read the time ROW (floats 20..22): ct' = +0, (-0) * (+0) = -0 and p + (-0) = p there too, so both keys are those of the
// centre that is drawn.
#ifndef GS4D_SLICE_RECORD_H
#define GS4D_SLICE_RECORD_H

#include <math.h>
#include "hd.h"

namespace gs4d_slicing {      // (gs4d_slice is the query structure of include/gs4d.h: a namespace cannot share its name)

// out (24 floats) <- the record in (24 floats) conditioned at time t; in and out must not overlap
GS4D_HD inline void record(float t, float min_opacity, float mu_t_out, float s44_out, const float in[24], float out[24]) {
    const float s44 = in[23];
    const float dt = t - in[3];
    const float inv = 1.0f / s44;
    const float e = expf(((-0.5f * dt) * inv) * dt);
    const float ot = e >= min_opacity ? e : min_opacity;           // the draw's maxf: a NaN e gives min_opacity
    const float k = inv * dt;
    const float a[3] = { in[11], in[15], in[19] };                 // the time COLUMN, as the draw reads it
    const float tv[3] = { inv * in[20], inv * in[21], inv * in[22] };      // the time row over Sigma44
    GS4D_UNROLL
    for (int r = 0; r < 3; ++r) out[r] = in[r] + (k * a[r]);
    out[3] = mu_t_out;
    GS4D_UNROLL
    for (int c = 4; c < 7; ++c) out[c] = in[c];
    out[7] = ot * in[7];
    GS4D_UNROLL
    for (int c = 0; c < 3; ++c) {
        GS4D_UNROLL
        for (int r = 0; r < 3; ++r) out[8 + 4 * c + r] = in[8 + 4 * c + r] - (a[r] * tv[c]);
        out[8 + 4 * c + 3] = -0.0f;                                // the time column
    }
    out[20] = -0.0f; out[21] = -0.0f; out[22] = -0.0f;             // the time row
    out[23] = s44_out;
}

} // namespace gs4d_slicing
#endif
