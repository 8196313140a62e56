// warp_record.h — one 96-byte SplatData record pushed through the linearisation, at its own centre, of the map x' = x + D(x) that a 4D lattice of
// displacement nodes gives by multilinear interpolation: the per-record text of gs4d_warp_records (include/gs4d.h) as plain C++ inline
// functions on top of transform_record.h — the one text of the definition.  csrc/warp.hip evaluates it on the device, host/gs4d_host.cpp
// (gs4d_host_warp_records) on the CPU; tests/warp_record_check.cpp compiles it stand-alone.  It follows the header's text operation by operation:
// float32, every product, sum and difference rounded on its own in the order the parentheses give (build without contraction), full products.
// `nodes` is whatever fetches a node: nodes(j, v) fills v[4] with (dx, dy, dz, dt) of node j; it is called for nodes of the lattice only, whatever
// the record, lo and inv hold — a centre that is not inside the lattice on every axis that takes part (a NaN never is) makes the record a copy
// before anything is converted to an integer or fetched.
#ifndef GS4D_WARP_RECORD_H
#define GS4D_WARP_RECORD_H

#include "pose_record.h"

namespace gs4d_warp {

constexpr unsigned int MAX_DIM = 65535u;                      // nodes along an axis, at most
constexpr unsigned long long MAX_NODES = 1ull << 28;          // nodes of a lattice, at most: 16 bytes each, every node index fits 32 bits

// the nodes of a lattice the call takes; 0 for one it refuses: a dim of 0 or above MAX_DIM, more than MAX_NODES nodes, clamp bits above 3, pad != 0
GS4D_HD inline unsigned long long node_count(const unsigned int dims[4], unsigned int clamp, const unsigned int pad[3]) {
    if ((clamp & ~15u) != 0u || pad[0] != 0u || pad[1] != 0u || pad[2] != 0u) return 0ull;
    unsigned long long count = 1ull;
    for (int a = 0; a < 4; ++a) {
        if (dims[a] == 0u || dims[a] > MAX_DIM) return 0ull;
        count *= dims[a];                                     // (<= 2^28 * 65535 before the test below: no overflow)
        if (count > MAX_NODES) return 0ull;
    }
    return count;
}

// where a centre stands in the lattice: its cell's first node and, per axis, the step to the cell's far node, the fraction, whether the axis takes
// part (d >= 2) and whether column a of G is +0 (d == 1, or the clamp changed u)
struct Cell {
    unsigned int base;
    unsigned int step[4];
    float f[4];
    bool two[4];
    bool flat[4];
};

// The cell of the centre p (floats 0..3 of a record).  False: p is not inside on an axis with d >= 2 — the record is copied, c is not to be used.
// The conversion to an integer stands behind the inside test: only 0 <= u <= d - 1 <= 65534 is ever converted.
GS4D_HD inline bool locate(const float lo[4], const float inv[4], const unsigned int dims[4], unsigned int clamp, const float p[4], Cell& c) {
    unsigned int stride = 1u;
    c.base = 0u;
    bool inside = true;
    GS4D_UNROLL
    for (int a = 0; a < 4; ++a) {
        const unsigned int d = dims[a];
        c.step[a] = stride;
        c.f[a] = 0.0f;
        c.two[a] = d >= 2u;
        c.flat[a] = true;
        if (d >= 2u) {
            float u = (p[a] - lo[a]) * inv[a];
            const float top = (float)(d - 1u);
            bool changed = false;
            if ((clamp >> a) & 1u) {
                if (u < 0.0f) { u = 0.0f; changed = true; }
                if (u > top) { u = top; changed = true; }
            }
            if (u >= 0.0f && u <= top) {
                unsigned int i = (unsigned int)u;
                if (i > d - 2u) i = d - 2u;
                c.f[a] = u - (float)i;
                c.flat[a] = changed;
                c.base += i * stride;
            } else {
                inside = false;
            }
        }
        stride *= d;
    }
    return inside;
}

// the interpolant reduced along the axes 0 .. A-1: the value v[k] of component k and g[a][k], its derivative along axis a < A
template <int A> struct Part {
    float v[4];
    float g[A > 0 ? A : 1][4];
};

// The fixed tree, reducing x, then y, then z, then t: o <- the part over the axes below A of the sub-lattice whose first node is j.  Level a = A-1
// takes the parts lo (at j) and hi (at j + step[a]) over the axes below it: the value step a + (f * (b - a)) on the value and on every derivative
// along an earlier axis, and (b - a) * inv[a] as the derivative along a.  A level whose axis has one node is skipped: lo as it is, hi never fetched.
// The recursion walks the nodes depth first, so every pair is reduced as soon as it is there.
template <int A, class Nodes>
GS4D_HD inline void sample(const Nodes& nodes, const float inv[4], const Cell& c, unsigned int j, Part<A>& o) {
    if constexpr (A == 0) {
        nodes(j, o.v);
    } else {
        constexpr int a = A - 1;
        Part<a> lo;
        sample<a>(nodes, inv, c, j, lo);
        if (!c.two[a]) {
            GS4D_UNROLL
            for (int k = 0; k < 4; ++k) { o.v[k] = lo.v[k]; o.g[a][k] = 0.0f; }
            GS4D_UNROLL
            for (int b = 0; b < a; ++b) {
                GS4D_UNROLL
                for (int k = 0; k < 4; ++k) o.g[b][k] = lo.g[b][k];
            }
            return;
        }
        Part<a> hi;
        sample<a>(nodes, inv, c, j + c.step[a], hi);
        const float f = c.f[a];
        GS4D_UNROLL
        for (int k = 0; k < 4; ++k) {
            const float d = hi.v[k] - lo.v[k];
            o.v[k] = lo.v[k] + (f * d);
            o.g[a][k] = d * inv[a];
        }
        GS4D_UNROLL
        for (int b = 0; b < a; ++b) {
            GS4D_UNROLL
            for (int k = 0; k < 4; ++k) o.g[b][k] = lo.g[b][k] + (f * (hi.g[b][k] - lo.g[b][k]));
        }
    }
}

// out (24 floats) <- the record in (24 floats) through the lattice (lo, inv, dims, clamp: the fields of a gs4d_lattice that node_count takes), or
// as it is when its centre is not inside; in and out must not overlap.  TIME: the tree has its t level; without it dims[3] must be 1 — both are the
// same definition, the level of an axis of one node being skipped.
template <bool TIME, class Nodes>
GS4D_HD inline void record(const Nodes& nodes, const float lo[4], const float inv[4], const unsigned int dims[4], unsigned int clamp,
                           const float in[24], float out[24]) {
    constexpr int AXES = TIME ? 4 : 3;
    Cell c;
    if (!locate(lo, inv, dims, clamp, in, c)) { gs4d_pose::copy(in, out); return; }
    Part<AXES> s;
    sample<AXES>(nodes, inv, c, c.base, s);
    // L = I + G, column-major; G[r][a] = d D_r / d x_a, a flat column is +0.0f
    float l[16];
    GS4D_UNROLL
    for (int a = 0; a < 4; ++a) {
        GS4D_UNROLL
        for (int r = 0; r < 4; ++r) {
            float g = 0.0f;
            if (a < AXES) g = c.flat[a] ? 0.0f : s.g[a < AXES ? a : 0][r];
            l[4 * a + r] = (r == a ? 1.0f : 0.0f) + g;
        }
    }
    // the mean: mu + D(mu)
    GS4D_UNROLL
    for (int r = 0; r < 4; ++r) out[r] = in[r] + s.v[r];
    // rgba
    GS4D_UNROLL
    for (int k = 4; k < 8; ++k) out[k] = in[k];
    gs4d_transform::sigma(l, in, out);
}

} // namespace gs4d_warp
#endif
