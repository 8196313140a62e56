// merge_record.h — the arithmetic of gs4d_cell_labels and gs4d_merge_records (include/gs4d.h) as plain C++ inline functions: the one
// text of the two definitions.  csrc/merge.hip evaluates it on the device, host/gs4d_host.cpp (gs4d_host_cell_labels, gs4d_host_merge_records) on
// the CPU, tests/merge_record_check.cpp stand-alone.  It restates the header's text operation by operation: area_time, mass and the cell in float32,
// the sums of a group in double, every product, difference, sum and quotient rounded on its own in the order the parentheses give (build without
// contraction), sqrtf and the divisions correctly rounded.  The record's Sigma: element (column c, row r) = float 8 + 4 * c + r; row / column 3 = time.
//
// Why a group's sums live in eight interleaved slots that are combined by one fixed tree: floating-point addition is not associative, so "the sum of
// a group" has bits only once its order is fixed.  Member k (in ascending record index) goes to slot k mod 8, a slot adds its members in ascending k,
// and the slots are combined as ((0+1)+(2+3))+((4+5)+(6+7)).  Eight lanes that walk members l, l + 8, ... each hold one slot, and a butterfly over
// lane distances 1, 2 and 4 is that tree in every lane, because x + y and y + x have the same bits.  A loop on one CPU thread gives the same bits.
#ifndef GS4D_MERGE_RECORD_H
#define GS4D_MERGE_RECORD_H

#include <math.h>
#include <stdint.h>
#include "hd.h"

namespace gs4d_merge {

constexpr uint32_t NONE = 0xFFFFFFFFu;                 // GS4D_ID_NONE: the label of a record that belongs to no group
constexpr int SLOTS = 8;                               // interleaved partial sums of a group
constexpr uint32_t MAX_DIM = 65536u;                   // cells along one axis at most
constexpr uint64_t MAX_CELLS = 0xFFFFFFFEull;          // cells of a grid at most: every label is below GS4D_ID_NONE

GS4D_HD inline bool finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

// ---- gs4d_cell_labels ----
// whether the device call takes the grid (reserved: the four reserved words)
GS4D_HD inline bool grid_ok(const float edge[4], const uint32_t dims[4], const uint32_t reserved[4]) {
    uint64_t cells = 1;
    for (int a = 0; a < 4; ++a) {
        if (dims[a] == 0u || dims[a] > MAX_DIM || reserved[a] != 0u) return false;
        if (dims[a] > 1u && !(finite(edge[a]) && edge[a] > 0.0f)) return false;
        cells *= dims[a];                                       // (<= 2^64: four factors of at most 2^16)
    }
    return cells <= MAX_CELLS;
}
// the label of a record whose rest mean is p = words 0..3, in a grid that grid_ok takes
GS4D_HD inline uint32_t cell_label(const float lo[4], const float edge[4], const uint32_t dims[4], const float p[4]) {
    uint32_t cell[4];
    GS4D_UNROLL
    for (int a = 0; a < 4; ++a) {
        cell[a] = 0u;
        if (dims[a] == 1u) continue;                            // the coordinate is not looked at
        const float g = (p[a] - lo[a]) / edge[a];
        if (g != g) return NONE;
        if (g >= 0.0f) cell[a] = (uint32_t)fminf(floorf(g), (float)(dims[a] - 1u));
    }
    return ((cell[3] * dims[2] + cell[2]) * dims[1] + cell[1]) * dims[0] + cell[0];
}

// ---- gs4d_merge_records: one record ----
GS4D_HD inline float area_time(const float rec[24]) {
    const float sxx = rec[8], syy = rec[13], szz = rec[18];
    const float e2 = ((sxx * syy - rec[12] * rec[9]) + (sxx * szz - rec[16] * rec[10])) + (syy * szz - rec[17] * rec[14]);
    return sqrtf(rec[23] * e2);
}
GS4D_HD inline float mass(const float rec[24]) { return rec[7] * area_time(rec); }
// what makes record `rec` a member beside its label and its table row: a finite mass > 0 (returned in a) and finite words 0..6 and 8..23
GS4D_HD inline bool member_mass(const float rec[24], float& a) {
    a = mass(rec);
    bool ok = finite(a) && a > 0.0f;
    GS4D_UNROLL
    for (int w = 0; w < 24; ++w) if (w != 7) ok = ok && finite(rec[w]);
    return ok;
}

// ---- gs4d_merge_records: the sums of a group ----
// Q holds the stored triangle r <= c in the order (0,0) (1,0) (1,1) (2,0) (2,1) (2,2) (3,0) (3,1) (3,2) (3,3) of (c, r)
struct Sums { double w, m[4], q[10], c[3]; };           // 18 doubles
GS4D_HD inline void clear(Sums& s) {
    s.w = 0.0;
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) s.m[r] = 0.0;
    GS4D_UNROLL
    for (int e = 0; e < 10; ++e) s.q[e] = 0.0;
    GS4D_UNROLL
    for (int j = 0; j < 3; ++j) s.c[j] = 0.0;
}
// member `rec` of mass a into its slot; origin: words 0..3 of the group's member 0
GS4D_HD inline void add_member(Sums& s, const float origin[4], float mass_a, const float rec[24]) {
    const double a = (double)mass_a;
    double d[4];
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) d[r] = (double)rec[r] - (double)origin[r];
    s.w += a;
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) s.m[r] += a * d[r];
    int e = 0;
    GS4D_UNROLL
    for (int c = 0; c < 4; ++c) {
        GS4D_UNROLL
        for (int r = 0; r <= c; ++r, ++e) s.q[e] += a * ((double)rec[8 + 4 * c + r] + d[r] * d[c]);
    }
    GS4D_UNROLL
    for (int j = 0; j < 3; ++j) s.c[j] += a * (double)rec[4 + j];
}
// x <- x + y, field by field: one node of the tree
GS4D_HD inline void join(Sums& x, const Sums& y) {
    x.w += y.w;
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) x.m[r] += y.m[r];
    GS4D_UNROLL
    for (int e = 0; e < 10; ++e) x.q[e] += y.q[e];
    GS4D_UNROLL
    for (int j = 0; j < 3; ++j) x.c[j] += y.c[j];
}
// the eight slots -> slot[0], by the tree ((0+1)+(2+3))+((4+5)+(6+7))
GS4D_HD inline void join_slots(Sums slot[SLOTS]) {
    for (int step = 1; step < SLOTS; step <<= 1)
        for (int s = 0; s < SLOTS; s += 2 * step) join(slot[s], slot[s + step]);
}
// the record of a group of two or more members from its combined sums
GS4D_HD inline void finish(const Sums& s, const float origin[4], float alpha_max, float out[24]) {
    double m[4];
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) { m[r] = s.m[r] / s.w; out[r] = (float)((double)origin[r] + m[r]); }
    GS4D_UNROLL
    for (int j = 0; j < 3; ++j) out[4 + j] = (float)(s.c[j] / s.w);
    int e = 0;
    GS4D_UNROLL
    for (int c = 0; c < 4; ++c) {
        GS4D_UNROLL
        for (int r = 0; r <= c; ++r, ++e) {
            const float v = (float)(s.q[e] / s.w - m[r] * m[c]);
            out[8 + 4 * c + r] = v;
            out[8 + 4 * r + c] = v;
        }
    }
    const double v = s.w / (double)area_time(out);             // (area_time reads words 8..23 only)
    out[7] = v < (double)alpha_max ? (float)v : alpha_max;      // a zero or NaN area: alpha_max
}

} // namespace gs4d_merge
#endif
