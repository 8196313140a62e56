// composite_common.h — what the two compositing kernels (composite.hip: ordered lists; composite2.hip: lists ordered in LDS) share.
#pragma once
#include "gs4d_internal.h"
#include <type_traits>

namespace gs4d {

// One chunk of <= 64 list entries is processed in one of two ways (wave-uniform choice):
//  * splat-parallel (small footprints, the 10^6..10^7-splat cube configs: a quad covers ~3 of the tile's 64 pixels):
//      phase A, lane = entry: evaluates the coverage rule only for the pixels of its own bounding box inside the tile and ORs its
//               bit into the per-pixel hit masks in LDS;
//      phase B, lane = pixel: walks the set bits of its own mask front to back, fetches that entry from LDS and blends.
//      Work is proportional to the number of covered pixels instead of 64 x entries.
//  * pixel-parallel broadcast (large footprints, e.g. the teapot scenes): every lane tests every entry of the chunk.
// Entries whose box inside the tile is wider or taller than SMALL_SIDE pixels are always tested pixel-parallel.
// (Round 2 walked each small box cell by cell up to 16 cells, x fastest, with a row wrap inside the loop: ~25 wave instructions per cell for
// three nested divergent regions.  A fixed SMALL_SIDE x SMALL_SIDE window walked by two UNIFORM loops — as many rows and columns as the
// widest box of the chunk has — needs no wrap and keeps everything of a row in registers: ~12 per cell.)
constexpr int SMALL_SIDE = 4;

// Workgroup -> tile.  Workgroups are dealt to the 8 XCDs round-robin (workgroup i runs on XCD i % 8) and each XCD has an L2 of its own;
// a splat that touches several tiles (1.38 entries per splat in the cube configs) is gathered once per tile.  With tile = workgroup id
// the tiles that share a record sit on different XCDs and every gather goes to memory.  Here the image is cut into blocks of 4 x 4
// tiles, block b belongs to XCD b % 8 (small blocks: the busy middle of the image is spread over all XCDs), and the workgroups of an
// XCD walk its blocks one after another: neighbours in the image are neighbours in time on one L2.
constexpr uint32_t XCDS = 8, TBLOCK = 4;
__host__ __device__ __forceinline__ uint32_t composite_grid(int tiles_x, int tiles_y) {
    const uint32_t nblocks = (uint32_t)((tiles_x + TBLOCK - 1) / TBLOCK) * (uint32_t)((tiles_y + TBLOCK - 1) / TBLOCK);
    return (nblocks + XCDS - 1) / XCDS * XCDS * (TBLOCK * TBLOCK);
}
__device__ __forceinline__ bool composite_tile(uint32_t wg, int tiles_x, int tiles_y, uint32_t& tile) {
    const uint32_t x = wg % XCDS, j = wg / XCDS;
    const uint32_t block = x + XCDS * (j / (TBLOCK * TBLOCK)), t = j % (TBLOCK * TBLOCK);
    const uint32_t bxn = (uint32_t)(tiles_x + TBLOCK - 1) / TBLOCK;
    const uint32_t tx = (block % bxn) * TBLOCK + (t % TBLOCK), ty = (block / bxn) * TBLOCK + (t / TBLOCK);
    tile = ty * (uint32_t)tiles_x + tx;
    return tx < (uint32_t)tiles_x && ty < (uint32_t)tiles_y;
}
// The same walk over a BOX of tiles (x0, y0, w, h — in tiles) of an image that is tiles_x tiles wide: the grid is composite_grid(w, h).
struct TileBox { uint32_t x0, y0, w, h; };
static_assert(TBLOCK == BOX_BLOCK, "a launch box is whole blocks of the compositor's walk");
// box: TileLists::box (blocks, inclusive; BOX_NONE = everything), clipped to the image
__host__ __device__ __forceinline__ TileBox tile_box(uint32_t box, int tiles_x, int tiles_y) {
    if (box == BOX_NONE) return TileBox{ 0u, 0u, (uint32_t)tiles_x, (uint32_t)tiles_y };
    const uint32_t x0 = box_x0(box) * BOX_BLOCK, y0 = box_y0(box) * BOX_BLOCK;
    const uint32_t x1 = (box_x1(box) + 1u) * BOX_BLOCK, y1 = (box_y1(box) + 1u) * BOX_BLOCK;
    const uint32_t cx1 = x1 < (uint32_t)tiles_x ? x1 : (uint32_t)tiles_x, cy1 = y1 < (uint32_t)tiles_y ? y1 : (uint32_t)tiles_y;
    return TileBox{ x0, y0, cx1 > x0 ? cx1 - x0 : 0u, cy1 > y0 ? cy1 - y0 : 0u };
}
__device__ __forceinline__ bool composite_tile(uint32_t wg, int tiles_x, TileBox box, uint32_t& tile) {
    uint32_t t;
    const bool real = composite_tile(wg, (int)box.w, (int)box.h, t);
    tile = (box.y0 + t / box.w) * (uint32_t)tiles_x + box.x0 + t % box.w;
    return real;
}

// glBlendFunc factors (GL enum values; the set the reference's menu offers, DebugMenus.h:41-59).  The reference never calls glBlendColor:
// the blend colour stays (0, 0, 0, 0), so CONSTANT_* = 0 and ONE_MINUS_CONSTANT_* = 1.
struct BlendFn { int sf, df; };
__device__ __forceinline__ float blend_factor(int f, float sc, float sa, float dc, float da) {
    switch (f) {
    case GS4D_ONE: case GS4D_ONE_MINUS_CONSTANT_COLOR: case GS4D_ONE_MINUS_CONSTANT_ALPHA: return 1.0f;
    case GS4D_SRC_COLOR: return sc;
    case GS4D_ONE_MINUS_SRC_COLOR: return 1.0f - sc;
    case GS4D_SRC_ALPHA: return sa;
    case GS4D_ONE_MINUS_SRC_ALPHA: return 1.0f - sa;
    case GS4D_DST_ALPHA: return da;
    case GS4D_ONE_MINUS_DST_ALPHA: return 1.0f - da;
    case GS4D_DST_COLOR: return dc;
    case GS4D_ONE_MINUS_DST_COLOR: return 1.0f - dc;
    default: return 0.0f;                                  // GS4D_ZERO, GS4D_CONSTANT_COLOR, GS4D_CONSTANT_ALPHA
    }
}
// dst = clamp(src * S + dst * D) on all four channels (OpenGL 4.4, 17.3.8: FUNC_ADD, fixed-point framebuffer; src is already clamped)
__device__ __forceinline__ void blend_general(BlendFn bf, float sr, float sg, float sb, float sa, float& dr, float& dg, float& db, float& da) {
    const float r = __saturatef(__fadd_rn(__fmul_rn(sr, blend_factor(bf.sf, sr, sa, dr, da)), __fmul_rn(dr, blend_factor(bf.df, sr, sa, dr, da))));
    const float g = __saturatef(__fadd_rn(__fmul_rn(sg, blend_factor(bf.sf, sg, sa, dg, da)), __fmul_rn(dg, blend_factor(bf.df, sg, sa, dg, da))));
    const float b = __saturatef(__fadd_rn(__fmul_rn(sb, blend_factor(bf.sf, sb, sa, db, da)), __fmul_rn(db, blend_factor(bf.df, sb, sa, db, da))));
    const float a = __saturatef(__fadd_rn(__fmul_rn(sa, blend_factor(bf.sf, sa, sa, da, da)), __fmul_rn(da, blend_factor(bf.df, sa, sa, da, da))));
    dr = r; dg = g; db = b; da = a;
}

// GENERAL = false: the default function (SRC_ALPHA, ONE_MINUS_SRC_ALPHA), accumulated front to back: colour C, transmittance T.
// GENERAL = true : any function of the menu, applied fragment by fragment in draw order to the pixel's value (Cr, Cg, Cb, A); T unused.
// exp(-32 q) as ONE multiply and the hardware's 2^x (v_exp_f32); [0, 1] clamps as one v_med3_f32 (finite arguments only reach them).
__device__ __forceinline__ float gauss_weight(float u, float v) { return __builtin_amdgcn_exp2f((u * u + v * v) * -46.16624130844683f); }      // -32 * log2(e)
__device__ __forceinline__ float clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }

// A pixel no fragment has reached holds the ID sentinel {ID_NONE, ID_NONE, 0.0f} (Outputs, gs4d_internal.h).
constexpr uint32_t ID_NONE = 0xFFFFFFFFu;

// What one pixel accumulates over one draw.  Default function: colour C and alpha A front to back, transmittance T; from Outputs::Aux on the
// weighted depth D; from Outputs::Ids on the draw's candidate (BW, BR) — the largest weight w > 0 so far and its record, the front-most of
// equal weights (walked front to back from BW = 0).  GENERAL: (Cr, Cg, Cb, A) is the pixel's value itself; T is unused.
// A level's kernels never read the members of the levels above it: they cost no register.  (BR stands first: the generated code sets the
// registers up in member order, and this order is the one the kernels had with loose locals.)
struct PixelAcc {
    uint32_t BR = ID_NONE;
    float T = 1.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, A = 0.0f, D = 0.0f, BW = 0.0f;
};

// d: the entry's depth (Outputs::Aux on, or ZTEST), rid: its record index (Outputs::Ids); a lane without a fragment blends with al = 0, so w = 0
// and it never becomes the candidate.  ZTEST: z is the pixel's value of the draw's depth-test plane; a fragment with d < z false (GL_LESS: a
// NaN hides) is hidden like a discarded one — al = 0 — so colour, aux and ID candidate all follow the test.
// STATS (record statistics, gs4d_set_record_stats): slot is the entry's count word in the chunk's stage (Stage::scnt(); its max and sum words lie
// STAT_PLANE and 2 * STAT_PLANE words behind it), inimg: the lane's pixel is inside the image.  A fragment with w > 0 there adds (1, bits of w,
// q(w)) with LDS atomics; any other lane adds 0 and takes the max with 0 — no branch.  q(w) = rint(w * 2^24) <= 2^24: 64 pixels fit 32 bits.
constexpr int STAT_PLANE = 64;
template <bool PREMULT_C, bool GENERAL, Outputs OUT, bool ZTEST, bool STATS = false>
__device__ __forceinline__ void blend_fragment(float u, float v, float alpha, float r_, float g_, float b_, PixelAcc& p, BlendFn bf, float d, uint32_t rid, float z,
                                               uint32_t* slot = nullptr, bool inimg = false) {
    static_assert(!GENERAL || (OUT == Outputs::Colour && !ZTEST), "aux and ID outputs and the depth test are defined for the default blend function only");
    static_assert(!STATS || (!GENERAL && OUT == Outputs::Colour && !ZTEST), "record statistics are built for the default blend function, colour only, no depth test");
    const float cg = gauss_weight(u, v);
    if (GENERAL) {
        if (cg >= 0.0001f) {                               // Splat4DFragShader.GLSL:30 discard
            const float al = clamp01(alpha * cg);
            if (PREMULT_C) { r_ = clamp01(r_ * cg); g_ = clamp01(g_ * cg); b_ = clamp01(b_ * cg); }
            blend_general(bf, r_, g_, b_, al, p.Cr, p.Cg, p.Cb, p.A);
        }
        return;
    }
    // The reference blends into a fixed-point (RGBA8) framebuffer: the GL clamps the fragment's colour and alpha to [0, 1] before the
    // blend (OpenGL 4.4, 17.3.8).  Colours that are not premultiplied were clamped once per record by the projection kernel.
    // No branch: a discarded fragment (Splat4DFragShader.GLSL:30) — and a lane that has no fragment at all, which passes alpha = 0 — blends
    // with al = 0, which leaves C and T as they are, exactly (C + 0 * c, T * 1).  The compositor is bound by instruction issue; a divergent
    // region costs four wave instructions whether or not a lane takes it.
    // (The depth test is one more compare in the same select.)
    const float al = (cg >= 0.0001f && (!ZTEST || d < z)) ? clamp01(alpha * cg) : 0.0f;
    const float w = p.T * al;
    if (PREMULT_C) { r_ = clamp01(r_ * cg); g_ = clamp01(g_ * cg); b_ = clamp01(b_ * cg); }   // Splat3DFragShaderFull.GLSL:22
    p.Cr += w * r_; p.Cg += w * g_; p.Cb += w * b_; p.A += w * al;
    if (has_aux(OUT)) p.D += w * d;
    if (has_ids(OUT)) { const bool take = w > p.BW; p.BW = take ? w : p.BW; p.BR = take ? rid : p.BR; }
    if constexpr (STATS) {
        const bool counts = inimg && w > 0.0f;
        __hip_atomic_fetch_add(slot, counts ? 1u : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_max(slot + STAT_PLANE, counts ? __float_as_uint(w) : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(slot + 2 * STAT_PLANE, counts ? (uint32_t)rintf(__fmul_rn(w, 16777216.0f)) : 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    p.T *= (1.0f - al);
}

// The end of a draw of the default blend function for the pixel at offset o: what the draw accumulated, composed over what the image holds
// with the colour's "over" (Outputs, gs4d_internal.h).  fb_is_clear (uniform): the tile is not in memory, it holds the clear values.
// The kernels call store_over, then (Outputs::Ids) id_over: with id_over nested in store_over the compiler orders six instructions differently.
// id_over, the ID triple (planes at ids, ids + P, ids + 2 P, P = W * H): the stored weight is scaled by the draw's final transmittance T, and the draw's
// candidate (BW, BR; BW == 0: none) replaces the triple when its weight is at least that (the newer draw is in front: ties go to it).
__device__ __forceinline__ void id_over(uint32_t* __restrict__ ids, size_t P, size_t o, bool fb_is_clear, float T, float BW, uint32_t BR, uint32_t draw) {
    uint32_t r = ID_NONE, dr = ID_NONE;
    float w = 0.0f;
    if (!fb_is_clear) { r = ids[o]; dr = ids[P + o]; w = __uint_as_float(ids[2 * P + o]); }
    w = T * w;
    const bool take = BW > 0.0f && BW >= w;
    ids[o] = take ? BR : r;
    ids[P + o] = take ? draw : dr;
    ids[2 * P + o] = __float_as_uint(take ? BW : w);
}
// store_over: the colour and (from Outputs::Aux on) the aux value
template <Outputs OUT>
__device__ __forceinline__ void store_over(const PixelAcc& p, size_t o, bool fb_is_clear, float4 clear, float4* fb, float2* aux) {
    const float4 d = fb_is_clear ? clear : fb[o];
    fb[o] = make_float4(p.Cr + p.T * d.x, p.Cg + p.T * d.y, p.Cb + p.T * d.z, p.A + p.T * d.w);
    if (has_aux(OUT)) {
        const float2 q = fb_is_clear ? make_float2(0.0f, 0.0f) : aux[o];
        aux[o] = make_float2(p.D + p.T * q.x, (1.0f - p.T) + p.T * q.y);
    }
}

// The LDS a chunk of <= 64 list entries is staged in: three float4 of every entry's projected record; from Outputs::Aux on, or with the depth
// test (ZTEST), the entries' depths (the last float of the same 64-byte record) behind them; from Outputs::Ids on their record indices behind
// those.  STATS: three more words per entry behind all that — fragments counted, bits of the largest w, sum of q(w) — zeroed when the chunk is
// staged and flushed to the draw's statistics buffer when it is done (composite_chunk).  A kernel gives it stage_words(OUT, ZTEST, STATS)
// words, 16-byte aligned.
constexpr bool stages_depth(Outputs o, bool ztest) { return has_aux(o) || ztest; }
constexpr int stage_words(Outputs o, bool ztest, bool stats = false) { return 64 * 3 * 4 + (stages_depth(o, ztest) ? 64 : 0) + (has_ids(o) ? 64 : 0) + (stats ? 3 * STAT_PLANE : 0); }
// (STATS also carries what only such a draw has — where its statistics go and whether the lane's pixel lies inside the image — set by the
// kernel once it knows its pixel.  They travel here, in an empty base of every other instance: as two more parameters of composite_chunk, even
// defaulted and unused, they move two instructions of every Ids instance.)
template <bool STATS> struct StageStats {};
template <> struct StageStats<true> { mutable StatOut so; mutable bool inimg = false; };
template <Outputs OUT, bool ZTEST, bool STATS = false>
struct Stage : StageStats<STATS> {
    float4* rec; float* depth; uint32_t* rid;
    __device__ __forceinline__ explicit Stage(float4* records) : rec(records), depth(stages_depth(OUT, ZTEST) ? reinterpret_cast<float*>(records + 64 * 3) : nullptr),
                                                                 rid(has_ids(OUT) ? reinterpret_cast<uint32_t*>(records + 64 * 3 + 16) : nullptr) {}
    // STATS: the entries' count words (no member: one more pointer in the struct moves two instructions of the Ids instances)
    __device__ __forceinline__ uint32_t* scnt() const { return reinterpret_cast<uint32_t*>(rec) + stage_words(OUT, ZTEST); }
};


// Host side of a launch: f(premultiplied colours?, output set, depth test?) with all three as compile-time constants (std::integral_constant).
template <class F>
inline void for_outputs(bool premult_c, Outputs out, bool ztest, F&& f) {
    auto with = [&](auto pc, auto zt) {
        switch (out) {
        case Outputs::Ids: f(pc, std::integral_constant<Outputs, Outputs::Ids>{}, zt); break;
        case Outputs::Aux: f(pc, std::integral_constant<Outputs, Outputs::Aux>{}, zt); break;
        default: f(pc, std::integral_constant<Outputs, Outputs::Colour>{}, zt); break;
        }
    };
    auto with_z = [&](auto pc) { if (ztest) with(pc, std::true_type{}); else with(pc, std::false_type{}); };
    if (premult_c) with_z(std::true_type{}); else with_z(std::false_type{});
}

// what blend_fragment is given beside the fragment: null / false unless STATS
template <Outputs OUT, bool ZTEST, bool STATS> __device__ __forceinline__ uint32_t* stat_slot(const Stage<OUT, ZTEST, STATS>& st, uint32_t e) { if constexpr (STATS) return st.scnt() + e; else return nullptr; }
template <Outputs OUT, bool ZTEST, bool STATS> __device__ __forceinline__ bool stat_inimg(const Stage<OUT, ZTEST, STATS>& st) { if constexpr (STATS) return st.inimg; else return false; }

// One chunk of the tile's list, front to back: lane s < cnt carries record `rec` of list entry (end of chunk - 1 - s), so s = 0 is the
// front-most entry.  GENERAL: the chunk is walked in DRAW order instead — lane s carries list entry (start of chunk + s).
// pmask: 64 x 2 words of LDS (per pixel: 64-bit mask of the chunk entries that cover it).  z: the lane's pixel's depth-test value (ZTEST).
// STATS: after the chunk's closing barrier lane s < cnt adds what its entry collected to the draw's statistics buffer (st.so), at so.rec[rec], if
// anything and if rec < so.n (a hostile sort index is data): one 32-bit add, one 32-bit max, one
// 64-bit add — relaxed, device scope, no return value.  One flush per (tile, chunk, entry), not per fragment.
template <bool PREMULT_C, bool GENERAL, Outputs OUT, bool ZTEST, bool STATS = false>
__device__ __forceinline__ void composite_chunk(const float4* __restrict__ proj, uint32_t rec, uint32_t cnt, uint32_t lane, int tx0, int ty0, float fx, float fy, const Stage<OUT, ZTEST, STATS>& st, uint32_t* pmask, int dbg,
                                                PixelAcc& acc, BlendFn bf, float z) {
    constexpr bool DEPTH = stages_depth(OUT, ZTEST);
    float4* const stage = st.rec;

    // lane s holds list entry hi-1-s : s = 0 is the LAST (front-most) entry of this chunk
    int lx0 = 0, ly0 = 0, bw = 0, bh = 0;
    float4 ra = make_float4(0, 0, 0, 0), rb = ra;
    if (lane < cnt) {
        const float4* r = proj + (size_t)rec * 4;
        ra = r[0]; rb = r[1];
        const float4 rc = r[2];
        stage[lane * 3 + 0] = ra;
        stage[lane * 3 + 1] = rb;
        stage[lane * 3 + 2] = rc;
        if (DEPTH) st.depth[lane] = reinterpret_cast<const float*>(r)[15];
        if (has_ids(OUT)) st.rid[lane] = rec;
        const uint32_t r0 = __float_as_uint(rc.z), r1 = __float_as_uint(rc.w);
        lx0 = max((int)(r0 & 0xFFFFu) - tx0, 0); ly0 = max((int)(r0 >> 16) - ty0, 0);
        const int lx1 = min((int)(r1 & 0xFFFFu) - tx0, TILE - 1), ly1 = min((int)(r1 >> 16) - ty0, TILE - 1);
        bw = lx1 - lx0 + 1;
        bh = ly1 - ly0 + 1;
        if (bw <= 0 || bh <= 0) { bw = 0; bh = 0; }            // no pixel of this tile (cannot happen for a list entry; kept exact)
    }
    const bool big = bw > SMALL_SIDE || bh > SMALL_SIDE;
    const uint64_t bigmask = __ballot(big);
    pmask[lane * 2] = 0u; pmask[lane * 2 + 1] = 0u;
    if constexpr (STATS) { st.scnt()[lane] = 0u; st.scnt()[STAT_PLANE + lane] = 0u; st.scnt()[2 * STAT_PLANE + lane] = 0u; }
    __syncthreads();
    if (dbg != 2 && (dbg == 1 || (uint32_t)__popcll(bigmask) * 2u > cnt)) {
        // ---- pixel-parallel broadcast over the whole chunk ----
        for (uint32_t s = 0; s < cnt; ++s) {
            const float4 a = stage[s * 3 + 0];          // cx, cy, a0x, a1x      (uniform address: LDS broadcast)
            const float4 b = stage[s * 3 + 1];          // a0y, a1y, r, g
            const float dx = __fsub_rn(fx, a.x), dy = __fsub_rn(fy, a.y);
            const float u = __fmaf_rn(a.z, dx, __fmul_rn(b.x, dy));
            const float v = __fmaf_rn(a.w, dx, __fmul_rn(b.y, dy));
            const bool cov = fabsf(u) <= 0.5f && fabsf(v) <= 0.5f;
            if (__ballot(cov) == 0ull) continue;
            const float4 c = stage[s * 3 + 2];          // b, alpha, -, -
            const float d = DEPTH ? st.depth[s] : 0.0f;
            const uint32_t rid = has_ids(OUT) ? st.rid[s] : 0u;
            if (cov) blend_fragment<PREMULT_C, GENERAL, OUT, ZTEST, STATS>(u, v, c.y, b.z, b.w, c.x, acc, bf, d, rid, z, stat_slot(st, s), stat_inimg(st));
        }
    } else {
        // ---- phase A (lane = entry): mark the covered pixels of small footprints ----
        // The box is at most SMALL_SIDE x SMALL_SIDE here.  Two uniform loops, over as many rows and columns as the tallest / widest small box
        // of the chunk: what does not change along a row stays in registers, and (float)(pixel) + 0.5f is formed afresh for every cell —
        // the same bits the pixel-parallel path and the checker use (pixel centres are integers + 0.5 below 2^16: exact).
        const int sw = big ? 0 : bw, sh = big ? 0 : bh;
        // the widest / tallest small box of the chunk, by ballots (scalar work: the vector pipe is the bottleneck here)
        int mw = 0, mh = 0;
#pragma unroll
        for (int k = 0; k < SMALL_SIDE; ++k) { if (__ballot(sw > k) != 0ull) mw = k + 1; if (__ballot(sh > k) != 0ull) mh = k + 1; }
        const float fx0 = (float)(tx0 + lx0) + 0.5f, fy0 = (float)(ty0 + ly0) + 0.5f;
        uint32_t* const pm0 = pmask + (ly0 * TILE + lx0) * 2 + (int)(lane >> 5);
        const uint32_t bit = 1u << (lane & 31u);
        float dxs[SMALL_SIDE];
#pragma unroll
        for (int xx = 0; xx < SMALL_SIDE; ++xx) dxs[xx] = __fsub_rn(fx0 + (float)xx, ra.x);
#pragma unroll
        for (int yy = 0; yy < SMALL_SIDE; ++yy) {
            if (yy >= mh) break;                            // uniform
            const float dyq = __fsub_rn(fy0 + (float)yy, ra.y);
            const float t0 = __fmul_rn(rb.x, dyq), t1 = __fmul_rn(rb.y, dyq);
            const bool rowin = yy < sh;
#pragma unroll
            for (int xx = 0; xx < SMALL_SIDE; ++xx) {
                if (xx >= mw) break;                        // uniform
                const float u = __fmaf_rn(ra.z, dxs[xx], t0);
                const float v = __fmaf_rn(ra.w, dxs[xx], t1);
                if (rowin && xx < sw && fabsf(u) <= 0.5f && fabsf(v) <= 0.5f) atomicOr(pm0 + (yy * TILE + xx) * 2, bit);
            }
        }
        // ---- large footprints of this chunk: every pixel tests them itself ----
        uint64_t mine = 0ull;
        for (uint64_t bm = bigmask; bm; bm &= bm - 1ull) {
            const int e = __ffsll((long long)bm) - 1;
            const float4 a = stage[e * 3 + 0];
            const float4 b = stage[e * 3 + 1];
            const float dx = __fsub_rn(fx, a.x), dy = __fsub_rn(fy, a.y);
            const float u = __fmaf_rn(a.z, dx, __fmul_rn(b.x, dy));
            const float v = __fmaf_rn(a.w, dx, __fmul_rn(b.y, dy));
            if (fabsf(u) <= 0.5f && fabsf(v) <= 0.5f) mine |= 1ull << e;
        }
        __syncthreads();
        // ---- phase B (lane = pixel): blend the entries that hit this pixel, front to back ----
        // One straight body per round (GENERAL keeps its branch: the blend functions of the menu are not the hot path): a pixel that has run
        // out of hits reads entry 0 and blends it with alpha 0 — nothing changes, and no divergent region is opened.
        uint64_t m = mine | (uint64_t)pmask[lane * 2] | ((uint64_t)pmask[lane * 2 + 1] << 32);
        while (__ballot(m != 0ull) != 0ull) {
            const bool on = m != 0ull;
            const int e = on ? __ffsll((long long)m) - 1 : 0;
            m &= m - 1ull;                                  // 0 stays 0
            const float4 a = stage[e * 3 + 0];
            const float4 b = stage[e * 3 + 1];
            const float4 c = stage[e * 3 + 2];
            const float dx = __fsub_rn(fx, a.x), dy = __fsub_rn(fy, a.y);
            const float u = __fmaf_rn(a.z, dx, __fmul_rn(b.x, dy));
            const float v = __fmaf_rn(a.w, dx, __fmul_rn(b.y, dy));
            if constexpr (GENERAL) { if (on) blend_fragment<PREMULT_C, true, OUT, false>(u, v, c.y, b.z, b.w, c.x, acc, bf, 0.0f, 0u, 0.0f); }
            else blend_fragment<PREMULT_C, false, OUT, ZTEST, STATS>(u, v, on ? c.y : 0.0f, b.z, b.w, c.x, acc, bf, DEPTH ? st.depth[e] : 0.0f, has_ids(OUT) ? st.rid[e] : 0u, z, stat_slot(st, (uint32_t)e), stat_inimg(st));
        }
    }
    __syncthreads();
    if constexpr (STATS) {
        const uint32_t n = st.scnt()[lane];                  // (the lane's own words: it zeroes them again when the next chunk is staged)
        if (lane < cnt && n != 0u && rec < st.so.n) {
            gs4d_record_stat* const o = st.so.rec + rec;
            __hip_atomic_fetch_add(&o->pixels, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(&o->wmax, st.scnt()[STAT_PLANE + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_add(&o->wsum, (uint64_t)st.scnt()[2 * STAT_PLANE + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

} // namespace gs4d
