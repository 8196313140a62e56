// preprocess.hip — per-splat vertex stage: 4D->3D time conditioning, EWA projection, 2x2 eigen-decomposition,
// window-space quad set-up.  One thread per splat, coalesced float4 loads from SoA planes, one 64-B projected
// record out.  Replaces the vertex shaders the reference runs 4x per splat (once per quad corner):
//   Shader/Splats4D/Splat4DVertexShaderInstanced.GLSL:81-150 (and ...Mod.GLSL:61-130)
//   Shader/Splats3D/Splat3DVertexShaderFull.GLSL:43-98
//   Shader/Splats2D/Splat2DVSI.GLSL:59-94
//
// Compiled with -ffp-contract=off and hipcc's default IEEE divide/sqrt: everything that decides pixel coverage
// (cx, cy, a0, a1) is bit-identical to the CPU checker, which evaluates the same expressions in the same order.
#include "gs4d_internal.h"
#include "footprint_rect.h"
#include "depth_key.h"
#include "proj_tile.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>

namespace gs4d {

// AoS 96-B SplatData (Scenes.h:22-37) -> planes.  Three layouts (SOA_*, gs4d_internal.h):
//   full      6 planes of float4: pos, col, sig[0], sig[1], sig[2], sig[3]                                                96 B / record
//   sym       pos, col, U = (s00, s01, s02, s11), V = sig[3] = (s03, s13, s23, s33) as float4 planes, W = (s12, s22) as a float2 plane   72 B / record
//   static3d  (px py pz s00), col, (s01 s02 s10 s11), (s12 s20 s21 s22): the 16 values of a STATIC 3D splat that differ from record to record   64 B / record
// sym holds a SYMMETRIC sig without its mirrored half — every covariance the reference's 4D scenes build is one (Splat.h:127, 141-154).
// static3d is for a set of 3D splats kept in the reference's 4D record: mu_t, sig's time column sig[c][3] and its time row sig[3][*] are
// the same eight values in every record (0, 0, 0, 0, (0, 0, 0, 1) for a 3D covariance: Scenes.h ObjectDisplay, the cube configs) and travel
// as kernel arguments.  Both are exact: the repack kernel compares what the layout assumes as bit patterns for every record and raises
// bbox[15] if any record breaks it; the host then repacks in the next layout down.  A third (a quarter) of the projection's read traffic is gone.
// float <-> unsigned with the same order, for atomicMin/atomicMax on floats
__device__ __forceinline__ uint32_t f2ord(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// Also reduces the bounding box of what the sort key depends on — position, mu_t and the velocity column sig[3].xyz
// (Scenes.h:28-36) — into bbox[0..6] = min, bbox[7..13] = max (order-preserving uint form), bbox[14] = non-finite input seen.
struct SoaConsts { float v[8]; };
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_soa_repack(const float4* __restrict__ aos, uint32_t n, float4* __restrict__ soa, uint32_t* __restrict__ bbox, SoaConsts cs) {
    constexpr bool COMPACT = LAYOUT != SOA_FULL;
    // one wave moves 64 records = 384 float4, read fully coalesced, written as 6 x 64 contiguous float4
    __shared__ float4 stage[4][384];
    __shared__ uint32_t red[4][16];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    // bounding box: accumulated in registers over the workgroup's whole share of the records, reduced once per workgroup, and only
    // then merged into the 15 global words (they share a cache line: one atomic per wave and chunk made the kernel 30x slower)
    uint32_t lo[7], hi[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) { lo[k] = 0xFFFFFFFFu; hi[k] = 0u; }
    bool bad = false, asym = false;
    for (uint32_t chunk = blockIdx.x; chunk * 256u < n; chunk += gridDim.x) {           // uniform trip count per workgroup
        const uint32_t rec0 = (chunk * 4u + w) * 64u;
        const uint32_t nrec = rec0 < n ? min(64u, n - rec0) : 0u;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            uint32_t f = j * 64u + lane;
            if (f < nrec * 6u) stage[w][f] = aos[(size_t)rec0 * 6u + f];
        }
        __builtin_amdgcn_wave_barrier();               // stage[w] is private to the wave
        if (lane < nrec) {
            auto same = [](float a, float b) { return __float_as_uint(a) == __float_as_uint(b); };
            if (LAYOUT == SOA_STATIC3D) {
                const float4 ps = stage[w][lane * 6u + 0], c0 = stage[w][lane * 6u + 2], c1 = stage[w][lane * 6u + 3], c2 = stage[w][lane * 6u + 4], c3 = stage[w][lane * 6u + 5];
                soa[rec0 + lane] = make_float4(ps.x, ps.y, ps.z, c0.x);
                soa[(size_t)n + rec0 + lane] = stage[w][lane * 6u + 1];
                soa[(size_t)2 * n + rec0 + lane] = make_float4(c0.y, c0.z, c1.x, c1.y);
                soa[(size_t)3 * n + rec0 + lane] = make_float4(c1.z, c2.x, c2.y, c2.z);
                if (!(same(ps.w, cs.v[0]) && same(c0.w, cs.v[1]) && same(c1.w, cs.v[2]) && same(c2.w, cs.v[3]) && same(c3.x, cs.v[4]) && same(c3.y, cs.v[5]) && same(c3.z, cs.v[6]) && same(c3.w, cs.v[7]))) asym = true;
            } else if (LAYOUT == SOA_SYM) {
                const float4 c0 = stage[w][lane * 6u + 2], c1 = stage[w][lane * 6u + 3], c2 = stage[w][lane * 6u + 4], c3 = stage[w][lane * 6u + 5];
                soa[rec0 + lane] = stage[w][lane * 6u + 0];
                soa[(size_t)n + rec0 + lane] = stage[w][lane * 6u + 1];
                soa[(size_t)2 * n + rec0 + lane] = make_float4(c0.x, c0.y, c0.z, c1.y);
                soa[(size_t)3 * n + rec0 + lane] = c3;
                reinterpret_cast<float2*>(soa + (size_t)4 * n)[rec0 + lane] = make_float2(c1.z, c2.z);
                // sig[c][r] == sig[r][c]: c0.y = sig[0][1] vs c1.x = sig[1][0], ...
                if (!(same(c0.y, c1.x) && same(c0.z, c2.x) && same(c0.w, c3.x) && same(c1.z, c2.y) && same(c1.w, c3.y) && same(c2.w, c3.z))) asym = true;
            } else {
#pragma unroll
                for (int p = 0; p < 6; ++p) soa[(size_t)p * n + rec0 + lane] = stage[w][lane * 6u + p];
            }
            const float4 ps = stage[w][lane * 6u + 0], s3 = stage[w][lane * 6u + 5];
            const float q[7] = { ps.x, ps.y, ps.z, ps.w, s3.x, s3.y, s3.z };
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                if (isfinite(q[k])) { const uint32_t o = f2ord(q[k]); lo[k] = min(lo[k], o); hi[k] = max(hi[k], o); }
                else bad = true;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int k = 0; k < 7; ++k) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { lo[k] = min(lo[k], (uint32_t)__shfl_xor(lo[k], off, 64)); hi[k] = max(hi[k], (uint32_t)__shfl_xor(hi[k], off, 64)); }
    }
    const bool anybad = __ballot(bad) != 0ull;
    if (COMPACT && __ballot(asym) != 0ull && lane == 0) atomicOr(&bbox[15], 1u);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) { red[w][k] = lo[k]; red[w][7 + k] = hi[k]; }
        red[w][14] = anybad ? 1u : 0u;
    }
    __syncthreads();
    if (threadIdx.x < 15u) {
        const uint32_t k = threadIdx.x;
        uint32_t v = red[0][k];
        for (int ww = 1; ww < 4; ++ww) v = k < 7u ? min(v, red[ww][k]) : k < 14u ? max(v, red[ww][k]) : (v | red[ww][k]);
        if (k < 7u) atomicMin(&bbox[k], v); else if (k < 14u) atomicMax(&bbox[k], v); else if (v) atomicOr(&bbox[14], 1u);
    }
}

hipError_t launch_soa_repack(hipStream_t st, const float* aos96, size_t n, float4* soa, uint32_t* bbox, const SoaInfo& info) {
    if (n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
    SoaConsts cs; for (int k = 0; k < 8; ++k) cs.v[k] = info.consts[k];
    if (info.layout == SOA_STATIC3D) k_soa_repack<SOA_STATIC3D><<<dim3(blocks), dim3(256), 0, st>>>((const float4*)aos96, (uint32_t)n, soa, bbox, cs);
    else if (info.layout == SOA_SYM) k_soa_repack<SOA_SYM><<<dim3(blocks), dim3(256), 0, st>>>((const float4*)aos96, (uint32_t)n, soa, bbox, cs);
    else k_soa_repack<SOA_FULL><<<dim3(blocks), dim3(256), 0, st>>>((const float4*)aos96, (uint32_t)n, soa, bbox, cs);
    return hipGetLastError();
}

// ---- shared device math (same expression order as the checker) ----------------------------------
struct PU { float V[16]; float P[16]; float time, min_opacity; int W, H; };

__device__ __forceinline__ float maxf_glsl(float a, float b) { return a >= b ? a : b; }
__device__ __forceinline__ void normalize2(float& x, float& y) { float tx = x * x, ty = y * y; float s = 1.0f / sqrtf(tx + ty); x = x * s; y = y * s; }

struct Quad { float e0x, e0y, e1x, e1y, s0, s1; };   // R columns and the S diagonal used in R*S

// GetEigenValues2x2 / GetEigenVectors2x2 / normalize (…Instanced.GLSL:59-78, 132-138)
__device__ __forceinline__ void eigen2(float u00, float u01, float u10, float u11, bool guard, float& lx, float& ly, Quad& q) {
    float m = (u00 + u11) * 0.5f;
    float p = (u00 * u11) - (u01 * u10);
    float d = sqrtf((m * m) - p);
    lx = maxf_glsl(m - d, 0.000001f);
    ly = maxf_glsl(m + d, 0.000001f);
    float ax, ay, bx, by;
    if (guard && u01 == 0.0f) { ax = 1.0f; ay = 0.0f; bx = 0.0f; by = 1.0f; }
    else {
        ax = u01; ay = lx - u00;
        normalize2(ax, ay);
        bx = ay; by = -ax;
        normalize2(ax, ay); normalize2(bx, by);
    }
    normalize2(ax, ay); normalize2(bx, by);
    q.e0x = ax; q.e0y = ay; q.e1x = bx; q.e1y = by;
}

__device__ __forceinline__ bool fin(float x) { return isfinite(x); }

// The projected record as its four 16-byte pieces, in the registers of the thread that projected it: emit() fills it, and its caller sends it to
// out.proj — by itself (store_record) or through its wave (proj_tile.h).
struct ProjRecord { float4 o[proj_tile::PIECES]; };
// every thread stores its own record: k_preprocess, and the k_project_count instances of a source that does not store through the wave (WAVE_STORE)
__device__ __forceinline__ void store_record(const PreOut& out, uint32_t i, const ProjRecord& p) {
    float4* o = out.proj + (size_t)i * 4;
#pragma unroll
    for (uint32_t k = 0; k < proj_tile::PIECES; ++k) o[k] = p.o[k];
}

// Window-space set-up + the record (into `p`: the caller stores it).  ncx,ncy = NDC centre; kx,ky = NDC scale of the quad offset; depth = -z_view of the centre (0: none).
__device__ __forceinline__ uint2 emit(const PreOut& out, uint32_t i, bool valid, const Quad& q, float ncx, float ncy, float kx, float ky,
                                      int W, int H, float r, float g, float b, float alpha, bool clamp_rgb, float depth, ProjRecord& p) {
    float cx = 0, cy = 0, a0x = 0, a0y = 0, a1x = 0, a1y = 0, hx = 0, hy = 0;
    uint32_t rect0 = 1u, rect1 = 0u;           // empty
    if (valid) {
        float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
        float sx = kx * hw, sy = ky * hh;
        cx = fmaf(ncx, hw, hw);
        cy = fmaf(ncy, hh, hh);
        float r0 = 1.0f / q.s0, r1 = 1.0f / q.s1;
        a0x = (q.e0x * r0) / sx; a0y = (q.e0y * r0) / sy;
        a1x = (q.e1x * r1) / sx; a1y = (q.e1y * r1) / sy;
        hx = 0.5f * (fabsf(q.e0x) * q.s0 + fabsf(q.e1x) * q.s1) * fabsf(sx);
        hy = 0.5f * (fabsf(q.e0y) * q.s0 + fabsf(q.e1y) * q.s1) * fabsf(sy);
        valid = fin(cx) && fin(cy) && fin(a0x) && fin(a0y) && fin(a1x) && fin(a1y) && fin(hx) && fin(hy) && fin(alpha);
        if (valid) {
            // conservative pixel rectangle: candidates are pixels whose centre lies within the bbox grown by a margin that
            // dominates the rounding of the coverage predicate
            float mx = 0.01f + 1e-5f * hx, my = 0.01f + 1e-5f * hy;
            // out.tight: the fragment test also discards what lies outside a disc of the quad's plane — the rectangle is the smaller of the
            // two boxes per axis (footprint_rect.h); hx, hy of the record stay the quad's
            float tx = hx, ty = hy;
            if (out.tight) gs4d_footprint::tighten(q.e0x, q.e0y, q.e1x, q.e1y, q.s0, q.s1, sx, sy, tx, ty);
            gs4d_footprint::pixel_rect(cx, cy, tx, ty, mx, my, W, H, rect0, rect1);
        }
    }
    if (!valid) { cx = cy = a0x = a0y = a1x = a1y = hx = hy = 0.0f; alpha = 0.0f; rect0 = 1u; rect1 = 0u; depth = 0.0f; }
    // the GL clamps a fragment's colour to [0, 1] before blending into the reference's RGBA8 framebuffer; where the fragment shader passes
    // the colour through unchanged that is a per-record operation (the 3D-Full shader multiplies by c first: clamped per fragment)
    // (fminf(fmaxf(x, 0), 1), the checker's form: a NaN colour clamps to 0 — __saturatef's compares let it through to every pixel of the footprint)
    if (clamp_rgb) { r = fminf(fmaxf(r, 0.0f), 1.0f); g = fminf(fmaxf(g, 0.0f), 1.0f); b = fminf(fmaxf(b, 0.0f), 1.0f); }
    // out.cull_alpha0 (a draw of the default blend function): a record whose alpha compares equal to 0 changes no pixel ("Records
    // that cannot change a pixel") — its record stays what it is, but the lists get no entry of it: the rectangle handed to the counting and
    // placing walks and the packed one are empty.  (The proof needs finite colours and a finite depth: w * y = 0 for w = 0.)
    uint32_t list0 = rect0, list1 = rect1;
    if (out.cull_alpha0 && alpha == 0.0f && fin(r) && fin(g) && fin(b) && fin(depth)) { list0 = 1u; list1 = 0u; }
    if (out.trects) out.trects[i] = pack_trect(list0, list1);      // (null: nothing downstream reads it — a staged draw writes its list entries itself)
    float4* const o = p.o;
    // (x components of the two affine rows side by side, likewise y: the compositor forms u and v with packed two-float instructions)
    o[0] = make_float4(cx, cy, a0x, a1x);
    o[1] = make_float4(a0y, a1y, r, g);
    o[2] = make_float4(b, alpha, __uint_as_float(rect0), __uint_as_float(rect1));
    // Nothing but gs4d_debug_read_projected and the compositor of a draw with aux outputs (the depth) reads the fourth float4 — and it is
    // written all the same: the record is one 64-byte line, and a line written whole goes to memory as it is, while a line with 16 bytes
    // missing has to be merged with what memory holds.  Measured with this store left out (round 3, 10^7 records): the projection kernel
    // 373 -> 459 us; at 10^6 records no difference (40.1 / 40.4 us).  (True whichever way the pieces leave: a wave that stores its records through
    // LDS, proj_tile.h, writes whole lines only because the fourth piece is among them.)
    o[3] = make_float4(hx, hy, valid ? 1.0f : 0.0f, out.aux ? depth : 0.0f);
    return make_uint2(list0, list1);
}

// Unordered draw path (tilelist.hip): the projection kernel also counts, per bucket b = tile % nb, the tile-list entries of the segment
// of records its workgroup walks (LDS atomics; the row of counts is stored once at the end) and stores each record's blend-order key.
// The wave's walk over the tiles of its 64 footprints: f(tile, key, rec) once per tile, with the key and the index of the record the tile belongs to.
// Called by all 64 lanes of the wave (`r.count` == 0 for lanes without a record): a lane walks a footprint of at most 16 tiles by itself; one of more is
// broadcast, record and key with it, and walked by the whole wave.
template <class F>
__device__ __forceinline__ void wave_for_each_tile(const TRect& r, uint32_t tiles_x, uint32_t key, uint32_t rec, F f) {
    const bool big = r.count > 16u;
    if (!big) for_each_tile(r, tiles_x, [&](uint32_t t) { f(t, key, rec); });
    uint64_t m = __ballot(big);
    const uint32_t lane = threadIdx.x & 63u;
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1ull;
        TRect rr;
        rr.tx0 = __shfl(r.tx0, src, 64); rr.ty0 = __shfl(r.ty0, src, 64); rr.wx = __shfl(r.wx, src, 64);
        rr.rows = __shfl(r.rows, src, 64); rr.tstep = __shfl(r.tstep, src, 64); rr.count = __shfl(r.count, src, 64);
        const uint32_t key2 = __shfl(key, src, 64), rec2 = __shfl(rec, src, 64);
        for (uint32_t j = lane; j < rr.count; j += 64u) f(tile_of(rr, j, tiles_x), key2, rec2);
    }
}
// first pass: the entries per bucket
__device__ __forceinline__ void count_buckets(uint32_t* h, uint32_t nbm, uint32_t tiles_x, const TRect& r) {
    wave_for_each_tile(r, tiles_x, 0u, 0u, [&](uint32_t t, uint32_t, uint32_t) { atomicAdd(&h[t & nbm], 1u); });
}
// Staged lists, second pass: the same walk again, every entry placed in the workgroup's LDS block at the position a returning LDS atomic on
// its bucket's cursor hands out (the cursors start at the scanned counts of the first pass).
__device__ __forceinline__ void place_buckets(uint32_t* cur, uint32_t nbm, uint32_t nbs, uint32_t tiles_x, const TRect& r, uint32_t key, uint32_t rec, uint2* stage) {
    wave_for_each_tile(r, tiles_x, key, rec, [&](uint32_t t, uint32_t k, uint32_t i) { stage[atomicAdd(&cur[t & nbm], 1u)] = make_uint2(k, ((t >> nbs) << 24) | i); });
}

// the depth key k_keygen (sort.hip) writes for this record, as a bit pattern relative to the host-proven lower bound
__device__ __forceinline__ uint32_t blend_key_4d(const KeySrc& ks, uint32_t i, const float4& p, const float4& s) {
    if (ks.mode == KEYSRC_INDEX) return i;
    const float key = ks.mode == KEYSRC_REF ? gs4d_key::ref_inv_euclid(p.x, p.y, p.z, p.w, s.x, s.y, s.z, ks.t, ks.camx, ks.camy, ks.camz)
                                            : gs4d_key::view_z(p.x, p.y, p.z, p.w, s.x, s.y, s.z, s.w, ks.t, ks.vr0, ks.vr1, ks.vr2, ks.vr3);
    return __float_as_uint(key) - ks.bias;
}

// …Instanced.GLSL:97-147 == Splat3DVertexShaderFull.GLSL:45-95.  C[c][r] = 3x3 covariance.
// depth: -z_view of the centre (what aux outputs accumulate), set whether or not the record survives the clip
__device__ __forceinline__ bool project3d(const PU& u, float mx, float my, float mz, const float C[3][3], Quad& q, float& ncx, float& ncy, float& depth) {
    const float* V = u.V; const float* P = u.P;
    float pcx = ((V[0] * mx + V[4] * my) + V[8] * mz) + V[12] * 1.0f;
    float pcy = ((V[1] * mx + V[5] * my) + V[9] * mz) + V[13] * 1.0f;
    float pcz = ((V[2] * mx + V[6] * my) + V[10] * mz) + V[14] * 1.0f;
    depth = -pcz;
    float pcw = ((V[3] * mx + V[7] * my) + V[11] * mz) + V[15] * 1.0f;
    float psx = ((P[0] * pcx + P[4] * pcy) + P[8] * pcz) + P[12] * pcw;
    float psy = ((P[1] * pcx + P[5] * pcy) + P[9] * pcz) + P[13] * pcw;
    float psz = ((P[2] * pcx + P[6] * pcy) + P[10] * pcz) + P[14] * pcw;
    float psw = ((P[3] * pcx + P[7] * pcy) + P[11] * pcz) + P[15] * pcw;
    float rw = 1.0f / psw;
    psx = rw * psx; psy = rw * psy; psz = rw * psz; psw = rw * psw;
    float z = psz / psw;
    float bound = 1.2f * psw;
    if (z < 0.0f || z > 1.0f || psx < -bound || psx > bound || psy < -bound || psy > bound) return false;
    if (!(fin(psx) && fin(psy) && fin(z))) return false;
    // gl_Position = uProj * vec4(R*S*v, 0, 1) + ps (:147): all four corners get z = ps.z + P[3][2] at w = 1, and the GL clips -w <= z <= w
    { const float zq = psz + P[14]; if (zq < -1.0f || zq > 1.0f) return false; }
    float z2 = pcz * pcz;
    float J[3][3] = { { 1.0f / pcz, 0.0f, -pcx / z2 }, { 0.0f, 1.0f / pcz, -pcy / z2 }, { 0.0f, 0.0f, 0.0f } };
    float Wt[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) Wt[c][r] = V[4 * r + c];
    float T[3][3], Tt[3][3], A[3][3], cov[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) T[c][r] = Wt[0][r] * J[c][0] + Wt[1][r] * J[c][1] + Wt[2][r] * J[c][2];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) Tt[c][r] = T[r][c];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) A[c][r] = Tt[0][r] * C[c][0] + Tt[1][r] * C[c][1] + Tt[2][r] * C[c][2];
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 2; ++r) cov[c][r] = A[0][r] * T[c][0] + A[1][r] * T[c][1] + A[2][r] * T[c][2];
    float lx, ly;
    eigen2(cov[0][0], cov[0][1], cov[1][0], cov[1][1], false, lx, ly, q);
    q.s0 = sqrtf(lx); q.s1 = sqrtf(ly);
    ncx = psx; ncy = psy;
    return true;
}

// One record each: returns its pixel rectangle, and through `key` its blend-order key (unordered path).
struct Src4D { const float4* soa; uint32_t stride; };      // six planes of `stride` float4 (the buffer's record count, not the draw's)
struct Src4DSym { const float4* soa; uint32_t stride; };   // the compact layout of a symmetric sig: pos, col, U, V as float4 planes, W as a float2 plane
struct Src4DStatic { const float4* soa; uint32_t stride; SoaConsts cs; };      // static 3D splats: four float4 planes, the time row / column of sig and mu_t as constants
struct Src3D { const float* verts; };
struct Src2D { const float* recs; };

__device__ __forceinline__ uint2 project_4d(const float4& pos, const float4& col, const float4& s0, const float4& s1, const float4& s2, const float4& s3,
                                            uint32_t i, const PU& u, const PreOut& out, const KeySrc& ks, uint32_t& key, ProjRecord& p);
// A record as loaded, before any of it is used: load_record issues all of a record's loads together, project_record(src, rec, ...) projects what they
// brought.  The staged loop of k_project_count loads round it + 1's record before it computes round it (the stores through PreOut may alias the source
// planes as far as the compiler knows: it hoists no load across them by itself).
struct Rec4D { float4 pos, col, s0, s1, s2, s3; };
struct Rec4DSym { float4 pos, col, U, V; float2 W; };
struct Rec4DStatic { float4 A, col, B, C; };
struct LoadHere {};      // no loaded record: project_record(src, LoadHere{}, ...) loads where it projects
__device__ __forceinline__ Rec4D load_record(const Src4D& src, uint32_t i) {
    const float4* __restrict__ soa = src.soa;
    const size_t ps = src.stride;
    Rec4D r;
    r.pos = soa[i]; r.col = soa[ps + i];
    r.s0 = soa[2 * ps + i]; r.s1 = soa[3 * ps + i]; r.s2 = soa[4 * ps + i]; r.s3 = soa[5 * ps + i];
    return r;
}
__device__ __forceinline__ Rec4DSym load_record(const Src4DSym& src, uint32_t i) {
    const float4* __restrict__ soa = src.soa;
    const size_t ps = src.stride;
    Rec4DSym r;
    r.pos = soa[i]; r.col = soa[ps + i]; r.U = soa[2 * ps + i]; r.V = soa[3 * ps + i];
    r.W = reinterpret_cast<const float2*>(soa + 4 * ps)[i];
    return r;
}
__device__ __forceinline__ Rec4DStatic load_record(const Src4DStatic& src, uint32_t i) {
    const float4* __restrict__ soa = src.soa;
    const size_t ps = src.stride;
    Rec4DStatic r;
    r.A = soa[i]; r.col = soa[ps + i]; r.B = soa[2 * ps + i]; r.C = soa[3 * ps + i];
    return r;
}
// arrived: from here on the record's registers hold what was loaded.  An empty statement that reads and "writes" every field: the compiler waits for the
// loads before it, and can move nothing that is computed from the record to before it.
__device__ __forceinline__ void arrived(float4& a) { asm volatile("" : "+v"(a.x), "+v"(a.y), "+v"(a.z), "+v"(a.w)); }
__device__ __forceinline__ void arrived(Rec4DStatic& r) { arrived(r.A); arrived(r.col); arrived(r.B); arrived(r.C); }
__device__ __forceinline__ void arrived(LoadHere&) {}
// load_ahead: what the staged loop requests a round ahead — the record of a static source, nothing of any other (their rounds load where they project).
// Measured (profiles/r11_experiments.txt items 3, 4): the static frame gains; the 96-byte source's kernel, six loads and 24 registers a round ahead,
// got 4 % slower alone and its frames showed no gain; the symmetric layout was left out untested, not because it failed (no workload of the benchmark reads it); Src3D and Src2D are never staged at scale.
__device__ __forceinline__ Rec4DStatic load_ahead(const Src4DStatic& src, uint32_t i) { return load_record(src, i); }
template <class SRC>
__device__ __forceinline__ LoadHere load_ahead(const SRC&, uint32_t) { return LoadHere{}; }
// WAVE_STORE: whether the k_project_count instances of a source send their records to out.proj through the wave's stage in LDS, as whole 64-byte lines
// (proj_tile.h), or every thread stores its own.  The stage costs an instance 6-8 VGPRs (profiles/r16_kernel_resources_*.txt): a source opts in where
// its instances keep their workgroups per CU and its frames gain — the static source does; the 96-byte source's staged instances
// would lose their third workgroup per CU, the symmetric one has no workload of the benchmark, Src3D and Src2D are never staged at scale.
// make lib PROJ_PLAIN_STORE=1: no source does (the measurement of round 16; never the shipped build).
template <class SRC> constexpr bool WAVE_STORE = false;
#if !defined(GS4D_PROJ_PLAIN_STORE)
template <> constexpr bool WAVE_STORE<Src4DStatic> = true;
#endif
__device__ __forceinline__ uint2 project_record(const Src4D&, const Rec4D& r, uint32_t, uint32_t i, const PU& u, const PreOut& out, const KeySrc& ks, uint32_t& key, ProjRecord& p) {
    return project_4d(r.pos, r.col, r.s0, r.s1, r.s2, r.s3, i, u, out, ks, key, p);
}
__device__ __forceinline__ uint2 project_record(const Src4DSym&, const Rec4DSym& r, uint32_t, uint32_t i, const PU& u, const PreOut& out, const KeySrc& ks, uint32_t& key, ProjRecord& p) {
    const float4& U = r.U; const float4& V = r.V; const float2& W = r.W;
    // sig[c] = column c; the mirrored elements are the same bits (verified by the repack kernel)
    return project_4d(r.pos, r.col, make_float4(U.x, U.y, U.z, V.x), make_float4(U.y, U.w, W.x, V.y), make_float4(U.z, W.x, W.y, V.z), V, i, u, out, ks, key, p);
}
__device__ __forceinline__ uint2 project_record(const Src4DStatic& src, const Rec4DStatic& r, uint32_t, uint32_t i, const PU& u, const PreOut& out, const KeySrc& ks, uint32_t& key, ProjRecord& p) {
    const float4& A = r.A; const float4& B = r.B; const float4& C = r.C;
    const float* c = src.cs.v;
    return project_4d(make_float4(A.x, A.y, A.z, c[0]), r.col, make_float4(A.w, B.x, B.y, c[1]), make_float4(B.z, B.w, C.x, c[2]), make_float4(C.y, C.z, C.w, c[3]), make_float4(c[4], c[5], c[6], c[7]),
                      i, u, out, ks, key, p);
}
// load, then project: what every caller that has no record in registers runs (the 4D sources; Src3D and Src2D read their record where they project, below)
template <class SRC>
__device__ __forceinline__ uint2 project_record(const SRC& src, LoadHere, uint32_t n, uint32_t i, const PU& u, const PreOut& out, const KeySrc& ks, uint32_t& key, ProjRecord& p) { return project_record(src, load_record(src, i), n, i, u, out, ks, key, p); }
__device__ __forceinline__ uint2 project_4d(const float4& pos, const float4& col, const float4& s0, const float4& s1, const float4& s2, const float4& s3,
                                            uint32_t i, const PU& u, const PreOut& out, const KeySrc& ks, uint32_t& key, ProjRecord& p) {
    float s44 = s3.w;
    float dt = u.time - pos.w;
    float ot = maxf_glsl(expf(-0.5f * dt * (1.0f / s44) * dt), u.min_opacity);     // :48-51, 83
    float ax = s0.w, ay = s1.w, az = s2.w;                                       // iSig[0][3], [1][3], [2][3]
    float k = (1.0f / s44) * dt;
    float mx = pos.x + k * ax, my = pos.y + k * ay, mz = pos.z + k * az;         // :86
    float inv = 1.0f / s44;
    float tv[3] = { inv * s3.x, inv * s3.y, inv * s3.z };                        // :87
    float a[3] = { ax, ay, az };
    float S[3][3] = { { s0.x, s0.y, s0.z }, { s1.x, s1.y, s1.z }, { s2.x, s2.y, s2.z } };
    float C[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) C[c][r] = S[c][r] - a[r] * tv[c];              // :89-95
    Quad q; float ncx = 0, ncy = 0, depth = 0;
    bool valid = project3d(u, mx, my, mz, C, q, ncx, ncy, depth);
    key = blend_key_4d(ks, i, pos, s3);
    return emit(out, i, valid, q, ncx, ncy, u.P[0], u.P[5], u.W, u.H, col.x, col.y, col.z, ot * col.w, true, depth, p);
}

__device__ __forceinline__ uint2 project_record(const Src3D& src, LoadHere, uint32_t, uint32_t i, const PU& u, const PreOut& out, const KeySrc&, uint32_t& key, ProjRecord& p) {
    const float* v = src.verts + (size_t)72 * i;      // vertex 0 of the quad: {vpos2, spos3, col4, sig9}
    float C[3][3];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int r = 0; r < 3; ++r) C[c][r] = v[9 + 3 * c + r];
    Quad q; float ncx = 0, ncy = 0, depth = 0;
    bool valid = project3d(u, v[2], v[3], v[4], C, q, ncx, ncy, depth);
    key = i;
    return emit(out, i, valid, q, ncx, ncy, u.P[0], u.P[5], u.W, u.H, v[5], v[6], v[7], v[8], false, depth, p);
}

__device__ __forceinline__ uint2 project_record(const Src2D& src, LoadHere, uint32_t, uint32_t i, const PU& u, const PreOut& out, const KeySrc&, uint32_t& key, ProjRecord& p) {
    const float* rec = src.recs + (size_t)12 * i;
    const float* P = u.P;
    float x = rec[0], y = rec[1];
    float psx = ((P[0] * x + P[4] * y) + P[8] * -1.0f) + P[12] * 1.0f;             // Splat2DVSI.GLSL:64
    float psy = ((P[1] * x + P[5] * y) + P[9] * -1.0f) + P[13] * 1.0f;
    float psz = ((P[2] * x + P[6] * y) + P[10] * -1.0f) + P[14] * 1.0f;
    float psw = ((P[3] * x + P[7] * y) + P[11] * -1.0f) + P[15] * 1.0f;
    float rw = 1.0f / psw;
    psx = rw * psx; psy = rw * psy; psz = rw * psz; psw = rw * psw;
    Quad q; float lx, ly;
    eigen2(rec[8], rec[9], rec[10], rec[11], true, lx, ly, q);
    float l0 = sqrtf(lx * 2.0f), l1 = sqrtf(ly * 2.0f);                           // :68-69
    q.s0 = l1; q.s1 = l0;                                                         // S = mat2(l1,0,0,l0) :76
    float zc = -5.0f + psz, wc4 = 1.0f + psw;
    float clipw = P[11] * zc + P[15] * wc4;
    float clipz = P[10] * zc + P[14] * wc4;
    bool valid = (clipw > 0.0f) && !(clipz < -clipw || clipz > clipw);
    float kx = P[0] / clipw, ky = P[5] / clipw;
    key = i;
    return emit(out, i, valid, q, kx * psx, ky * psy, kx, ky, u.W, u.H, rec[4], rec[5], rec[6], rec[7], true, 0.0f, p);     // 2D records have no depth
}

// One thread per record (the ordered path).
template <class SRC>
__global__ __launch_bounds__(256) void k_preprocess(SRC src, uint32_t n, PU u, PreOut out, TileCount tc) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t key;
    ProjRecord p;
    (void)project_record(src, LoadHere{}, n, i, u, out, tc.ks, key, p);
    store_record(out, i, p);
}

// ---- k_project_count: a workgroup projects one segment of the records, and does what the form asks beside (TileCount, gs4d_internal.h) ----
// lists Count, Stage (the unordered path): workgroup w walks records [w * seg, (w + 1) * seg), SEG_THREADS per round, and leaves the counts of its segment
// per bucket.
// keys Write, SegmentFed: it is also k_keygen (sort.hip) for these records — the key it derives the blend order from IS the depth key: written to the
// caller's key buffer with the identity index beside it, bounds-checked, and counted into the depth sort's digit histograms.  With lists None
// that is all it adds to the projection: the ordered path's form (the sort follows, then binning.hip reads the sorted index).
// Segment-fed depth sort (keys SegmentFed): the keys do not go to the caller's buffer.  The workgroup ranks them by their 9-bit top digit
// and writes them, with their record indices, digit after digit into the segment's block, for k_os_tail to gather (sort.hip).
static_assert(SEGFEED_BLOCK == (uint32_t)(STAGE_R * SEG_THREADS) && SEG_THREADS / 64 == 8 && OS_MAX_PASSES == 4, "segment-fed keys: a block per staged segment; eight waves' counters, four of them in kh");

// The workgroup's LDS.  stage[] is the dynamic part — lists Stage: tc.scap list entries.  A segment-fed producer has all of it free until the list entries are
// placed, and kh as well (it counts no histogram row there): per-wave digit counters [8][512] in kh (waves 0..3) and stage[0, 8 KB) (waves 4..7), the
// reordered pairs in stage[8 KB, 24 KB) — launch_segments asks for at least SEGFEED_LDS bytes of stage[].
constexpr size_t SEGFEED_COUNTERS = (4 * OS_MAX_BINS) * 4;                             // bytes of stage[]: the counters of waves 4..7
constexpr size_t SEGFEED_LDS = SEGFEED_COUNTERS + (size_t)SEGFEED_BLOCK * 8;           // ... then the pairs
// A source with WAVE_STORE: during the rounds stage[] also holds the eight waves' record stages (proj_tile.h) — from its first byte, or behind the counters of a
// segment-fed producer, which are live then.  Everything else of stage[] is written only behind the barrier that ends the rounds.
constexpr size_t WAVE_STAGES_BYTES = proj_tile::stage_bytes(SEG_THREADS / 64, proj_tile::PITCH);
constexpr size_t wave_stages_at(bool segf) { return segf ? SEGFEED_COUNTERS : 0; }
struct ProjLds {
    uint32_t* h;                        // lists: the segment's entries per bucket; placing pass: the buckets' cursors
    uint32_t (*kh)[OS_MAX_BINS];        // keys Write: the digit histograms (os_hist_*); keys SegmentFed: the digit counters of waves 0..3
    uint32_t* ws;                       // the wave sums of a block scan
    uint2* stage;
    float4* records;                    // WAVE_STORE: this wave's stage for the records of a round (proj_tile.h), laid over stage[] — which is idle during the rounds but for the
                                        // segment-fed form's counters, and the stages stand behind those (wave_stages_at)
    __device__ __forceinline__ uint32_t* stage32() const { return reinterpret_cast<uint32_t*>(stage); }
    __device__ __forceinline__ uint32_t* wave_row(uint32_t k) const { return k < 4u ? kh[k] : stage32() + (k - 4u) * OS_MAX_BINS; }      // segment-fed: the digit counters of wave k
    __device__ __forceinline__ uint2* pairs() const { return stage + SEGFEED_COUNTERS / sizeof(uint2); }                                  // segment-fed: the reordered pairs
};

// Round `it` of a staged segment [i0, i1): thread t takes record i0 + it * SEG_THREADS + t.  Segment-fed: a wave owns 256 CONSECUTIVE records, four rounds of 64 —
// (wave, round, lane) order is then record order, which is what makes the placing of the pairs stable (os_rank_items' layout).  Every round of a wave starts
// at a multiple of 64: a wave is either wholly past the end of the segment (it leaves the loop: wave-uniform, no barrier inside) or stays converged.
template <bool SEGF>
struct StagedRounds {
    uint32_t i0, i1, wave;
    __device__ __forceinline__ uint32_t first(int it) const { return SEGF ? i0 + wave * (uint32_t)(STAGE_R * 64) + (uint32_t)it * 64u : i0 + (uint32_t)it * SEG_THREADS; }
    __device__ __forceinline__ uint32_t lane() const { return SEGF ? (threadIdx.x & 63u) : threadIdx.x; }
    __device__ __forceinline__ uint32_t record(int it) const { return first(it) + lane(); }              // the record this thread projects in round `it`
    __device__ __forceinline__ uint32_t ahead(int it) const { return min(record(it), i1 - 1u); }         // ... and the one it requests for it: never beyond the segment's last
};
// staged lists: what the placing pass needs of every record this thread projected (seg <= STAGE_R * SEG_THREADS: tile_lists_plan / run_draw)
template <int R> struct KeptRecords { uint32_t key[R], r0[R], r1[R]; };

// One round of one record per thread (rec: loaded earlier, or LoadHere): project it, keep {key, rectangle} for the placing pass, write or count its depth key,
// count its list entries per bucket.  Every lane stays for the wave-wide counting.
template <ProjLists LISTS, ProjKeys KEYS, class SRC, class REC, int R>
__device__ __forceinline__ void project_round(const SRC& src, const REC& rec, uint32_t n, uint32_t i, uint32_t i1, int it, uint32_t wave, const PU& u, const PreOut& out,
                                              const TileCount& tc, const ProjLds& lds, KeptRecords<R>& kept) {
    TRect r{ 0u, 0u, 0u, 0u, 1u, 0u };
    uint32_t key = 0u;
    const uint32_t lane = threadIdx.x & 63u;
    if (i < i1) {
        ProjRecord p;
        const uint2 rect = project_record(src, rec, n, i, u, out, tc.ks, key, p);
        if constexpr (WAVE_STORE<SRC>) proj_tile::put_record(lds.records, lane, p.o); else store_record(out, i, p);
        if constexpr (LISTS != ProjLists::None) {
            if (LISTS == ProjLists::Count && KEYS == ProjKeys::None) tc.skey[i] = key;               // fused: k_bucket_scatter takes the key from the caller's key buffer, written just below
            r = tile_rect(rect.x, rect.y, (uint32_t)tc.shard_rank, (uint32_t)tc.shard_world);
            if constexpr (LISTS == ProjLists::Stage) { kept.key[it] = key; kept.r0[it] = rect.x; kept.r1[it] = rect.y; }
        }
        if constexpr (KEYS != ProjKeys::None) {
            if constexpr (KEYS == ProjKeys::SegmentFed) {
                atomicAdd(&lds.wave_row(wave)[(key >> tc.hist_top) & (OS_MAX_BINS - 1u)], 1u);      // the wave's count of the digit; the slot comes from a second walk (segfeed_epilogue)
            } else {
                tc.keys_out[i] = __uint_as_float(key + tc.ks.bias);      // the blend key is the depth key's bit pattern relative to the bias
                if (tc.idx_out) tc.idx_out[i] = i;                        // null: the sort that follows makes up the identity payload itself (radix_sort_pairs)
            }
            if (key > tc.span) __hip_atomic_store(tc.err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // below the bias wraps to a huge value: caught too
        }
    }
    if constexpr (WAVE_STORE<SRC>) {
        // All 64 lanes are here, and lane 0's record is a multiple of 64 in every form (a segment starts at a multiple of SEG_THREADS, a round and a wave's share of it
        // at multiples of 64): the wave's records below i1 are one contiguous piece of out.proj, and leave as whole lines.  Wave-level ordering is all it takes.
        const uint32_t first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(i - lane));
        proj_tile::wave_sync();
        proj_tile::store_staged(out.proj + (size_t)first * proj_tile::PIECES, lds.records, lane, proj_tile::wave_have(first, i1));
        proj_tile::wave_sync();      // the next round's puts stay behind these reads
    }
    if constexpr (KEYS == ProjKeys::Write) os_hist_add(lds.kh, key, i < i1, tc.hist_rows, tc.hist_rb, tc.hist_top);       // a hybrid-planned sort: the top-digit row alone (one LDS atomic per record, not three)
    if constexpr (LISTS != ProjLists::None) count_buckets(lds.h, tc.nb - 1u, (uint32_t)tc.tiles_x, r);
}

// Segment-fed keys, after the rounds: the segment's (key, record) pairs leave grouped by top digit, stable in record order.
__device__ __forceinline__ void segfeed_epilogue(const TileCount& tc, const StagedRounds<true>& sr, const ProjLds& lds, const KeptRecords<STAGE_R>& kept) {
    // thread d: the waves' counts of digit d -> each wave's first slot inside the block (digit runs in order, waves in order inside a run), the run-table
    // word and the global top-digit histogram (what os_hist_flush would have added)
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    uint32_t wo[SEG_THREADS / 64], cnt = 0;
#pragma unroll
    for (int k = 0; k < SEG_THREADS / 64; ++k) { wo[k] = cnt; cnt += lds.wave_row((uint32_t)k)[tid]; }
    const uint32_t inc = wave_incl_scan_u32(cnt, lane);
    if (lane == 63u) lds.ws[sr.wave] = inc;
    __syncthreads();
    uint32_t first = inc - cnt;
#pragma unroll
    for (int k = 0; k < SEG_THREADS / 64; ++k) if ((unsigned)k < sr.wave) first += lds.ws[k];
#pragma unroll
    for (int k = 0; k < SEG_THREADS / 64; ++k) lds.wave_row((uint32_t)k)[tid] = first + wo[k];
    tc.seg_runs[(size_t)tid * tc.rows + blockIdx.x] = cnt | (first << 12);      // both <= SEGFEED_BLOCK
    if (cnt) atomicAdd(&tc.ghist[((size_t)(blockIdx.x % OS_REPL) * OS_MAX_PASSES + OS_TOP_ROW) * OS_MAX_BINS + tid], cnt);
    __syncthreads();
    uint2* const pairs = lds.pairs();
    uint32_t* const mine = lds.wave_row(sr.wave);
#pragma unroll
    for (int q = 0; q < STAGE_R; ++q) {
        const uint32_t i = sr.first(q) + lane;
        // Stable without a stored rank: the counter now holds the wave's next free slot of the digit, and a returning LDS atomic hands the slots out to the
        // lanes of one instruction in ascending lane order (verified on the device at context creation — the hybrid is planned only then: os_rank_items),
        // instruction after instruction in program order — rounds in order, lanes in order inside a round: record order.
        if (i < sr.i1) pairs[atomicAdd(&mine[(kept.key[q] >> tc.hist_top) & (OS_MAX_BINS - 1u)], 1u)] = make_uint2(kept.key[q] + tc.ks.bias, i);
    }
    __syncthreads();
    // the block leaves in one piece, 16 bytes (two pairs) per thread and step; a segment of an odd number of records also stores the slot behind its last pair
    uint4* __restrict__ dst = reinterpret_cast<uint4*>(tc.seg_pairs + (size_t)blockIdx.x * SEGFEED_BLOCK);
    const uint4* src4 = reinterpret_cast<const uint4*>(pairs);
    for (uint32_t k = tid; k < (sr.i1 - sr.i0 + 1u) / 2u; k += SEG_THREADS) dst[k] = src4[k];
    // (ws and stage[] are written again by count_epilogue: behind the barriers of its scan, which every thread reaches after the loop above)
}

// Lists, after the rounds: the row of counts (one row per bucket: k_bucket_scan / k_bucket_tiles_staged walk along the segments), the segment's total and — staged —
// the exclusive scan of the counts: where each bucket's run starts inside the segment's block; then the entries are placed there and the block stored.
// Thread t looks after buckets 2t, 2t + 1.
template <ProjLists LISTS, class ROUNDS, int R>
__device__ __forceinline__ void count_epilogue(const TileCount& tc, const ROUNDS& sr, const ProjLds& lds, const KeptRecords<R>& kept) {
    uint32_t* const h = lds.h;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6, b0 = 2u * tid;
    const uint32_t c0 = b0 < tc.nb ? h[b0] : 0u, c1 = b0 + 1u < tc.nb ? h[b0 + 1u] : 0u, sum = c0 + c1;
    // (written out, not wave_incl_scan_u32: with the call here two of the static staged instances allocate other registers, profiles/r12_kernel_resources_*.txt)
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const uint32_t v = __shfl_up(inc, off, 64); if (lane >= (unsigned)off) inc += v; }
    if (lane == 63u) lds.ws[w] = inc;
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int k = 0; k < SEG_THREADS / 64; ++k) { const uint32_t v = lds.ws[k]; if ((unsigned)k < w) base += v; total += v; }
    const uint32_t o0 = base + inc - sum, o1 = o0 + c0;
    if (b0 < tc.nb) tc.hist[(size_t)b0 * tc.rows + blockIdx.x] = c0;
    if (b0 + 1u < tc.nb) tc.hist[(size_t)(b0 + 1u) * tc.rows + blockIdx.x] = c1;
    if (tid == 0u) tc.sstat[blockIdx.x] = total;
    if constexpr (LISTS == ProjLists::Stage) {
        if (b0 < tc.nb) { tc.offs[(size_t)b0 * tc.rows + blockIdx.x] = o0; h[b0] = o0; }
        if (b0 + 1u < tc.nb) { tc.offs[(size_t)(b0 + 1u) * tc.rows + blockIdx.x] = o1; h[b0 + 1u] = o1; }
        const bool fits = total <= tc.scap;            // uniform (every thread added up the same ws[])
        if (!fits && tid == 0u) *tc.abort_word = tc.seq;      // the block cannot hold this segment: the draw is re-run with exact lists (every writer stores the same value)
        __syncthreads();
        if (fits) {
            const uint32_t nbs = (uint32_t)__ffs((int)tc.nb) - 1u;
#pragma unroll
            for (int q = 0; q < STAGE_R; ++q) {
                const uint32_t i = sr.record(q);                          // the record this thread projected in round q
                if (sr.first(q) >= sr.i1) break;                          // uniform in the wave
                const TRect r = i < sr.i1 ? tile_rect(kept.r0[q], kept.r1[q], (uint32_t)tc.shard_rank, (uint32_t)tc.shard_world) : TRect{ 0u, 0u, 0u, 0u, 1u, 0u };
                place_buckets(h, tc.nb - 1u, nbs, (uint32_t)tc.tiles_x, r, kept.key[q], i, lds.stage);
            }
            __syncthreads();
            // the block leaves the workgroup in one piece: consecutive threads, consecutive 16-byte pieces
            uint4* __restrict__ dst = reinterpret_cast<uint4*>(tc.stage_out + (size_t)blockIdx.x * tc.scap);
            const uint4* src4 = reinterpret_cast<const uint4*>(lds.stage);
            for (uint32_t k = tid; k < (total + 1u) / 2u; k += SEG_THREADS) dst[k] = src4[k];
        }
    }
}

// SegmentFed: the segment-fed form of <SRC, Stage, Write> — an instance of its own, so that the others keep their registers
template <class SRC, ProjLists LISTS, ProjKeys KEYS>      // the form: TileCount::lists, TileCount::keys
__global__ __launch_bounds__(SEG_THREADS) void k_project_count(SRC src, uint32_t n, PU u, PreOut out, TileCount tc) {
    constexpr bool COUNTS = LISTS != ProjLists::None, STAGES = LISTS == ProjLists::Stage, KEYED = KEYS != ProjKeys::None, SEGF = KEYS == ProjKeys::SegmentFed;
    static_assert(!SEGF || STAGES, "segment-fed keys come from the staged, fused projection");
    __shared__ uint32_t h[COUNTS ? 1024 : 1];
    __shared__ uint32_t kh[KEYED ? OS_MAX_PASSES : 1][OS_MAX_BINS];
    __shared__ uint32_t ws[SEG_THREADS / 64 + 1];
    extern __shared__ __attribute__((aligned(16))) uint2 stage[];      // (copied out 16 bytes at a time: 16-byte base)
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float4* const records = WAVE_STORE<SRC> ? reinterpret_cast<float4*>(reinterpret_cast<char*>(stage) + wave_stages_at(SEGF)) + proj_tile::record_slot(wave * proj_tile::WAVE, proj_tile::PITCH) : nullptr;
    const ProjLds lds{ h, kh, ws, stage, records };
    if (COUNTS) for (uint32_t b = threadIdx.x; b < tc.nb; b += SEG_THREADS) h[b] = 0u;
    if (KEYED && threadIdx.x < 256u) os_hist_clear(kh, threadIdx.x);
    if (SEGF) for (uint32_t q = threadIdx.x; q < SEGFEED_COUNTERS / 4; q += SEG_THREADS) lds.stage32()[q] = 0u;
    __syncthreads();
    const uint32_t i0 = blockIdx.x * tc.seg, i1 = min(n, i0 + tc.seg);
    const StagedRounds<SEGF> sr{ i0, i1, wave };
    KeptRecords<STAGES ? STAGE_R : 1> kept;
#pragma unroll
    for (int q = 0; q < (STAGES ? STAGE_R : 1); ++q) { kept.key[q] = 0u; kept.r0[q] = 1u; kept.r1[q] = 0u; }
    if constexpr (STAGES) {
        // The rounds of a staged segment, with their look-ahead.
        // Software-pipelined (sources with a load_ahead of their own): round it + 1's record is requested before anything of round it is computed, and arrives while round it projects, stores
        // and counts.  No address at or beyond the segment's end is ever formed (the last plane of a buffer as long as the draw ends exactly there): a
        // lane whose record lies at or past i1, and every lane of a round that does not exist, asks for the segment's last record, i1 - 1 >= i0, again (StagedRounds::ahead) —
        // a line its wave or its neighbour has just had — and project_round projects nothing for it.  The request stands under no branch on purpose: under
        // either guard of the round the compiler merges the registers being loaded with "not loaded" where the branch ends, copies them there, and waits
        // for the loads in front of the copies — where they were issued (profiles/r11_experiments.txt item 2).
        // rec[it] is written by request(it) alone and read by round it alone, and two are live at a time.  arrived() marks where round it starts: the
        // wait for its record stands there, behind round it - 1's stores, and nothing computed from the record can be moved up into round it - 1.
        // (The loop stands here, and request is a lambda: as a function of its own, or with the assignment written out, every staged instance allocates other
        // registers — the static ones 26 fewer — profiles/r12_kernel_resources_*.txt.)
        decltype(load_ahead(src, 0u)) rec[STAGE_R];
        auto request = [&](int it) { rec[it] = load_ahead(src, sr.ahead(it)); };
        request(0);
#pragma unroll
        for (int it = 0; it < STAGE_R; ++it) {      // trip count uniform in the wave, registers indexed at compile time
            const uint32_t ib = sr.first(it);
            if (ib >= i1) break;
            const uint32_t i = ib + sr.lane();
            arrived(rec[it]);
            if (it + 1 < STAGE_R) request(it + 1);
            project_round<LISTS, KEYS>(src, rec[it], n, i, i1, it, wave, u, out, tc, lds, kept);
        }
    }
    else for (uint32_t ib = i0; ib < i1; ib += SEG_THREADS) project_round<LISTS, KEYS>(src, LoadHere{}, n, ib + threadIdx.x, i1, 0, wave, u, out, tc, lds, kept);    // uniform trip count
    __syncthreads();
    if constexpr (SEGF) segfeed_epilogue(tc, sr, lds, kept);
    if constexpr (COUNTS) count_epilogue<LISTS>(tc, sr, lds, kept);
    if constexpr (KEYS == ProjKeys::Write) if (threadIdx.x < 256u) os_hist_flush(kh, tc.ghist, tc.hist_rows, threadIdx.x, tc.hist_top);
}

static PU make_pu(const Uniforms& un, int W, int H) {
    PU u;
    for (int i = 0; i < 16; ++i) { u.V[i] = un.view[i]; u.P[i] = un.proj[i]; }
    u.time = un.time; u.min_opacity = un.min_opacity; u.W = W; u.H = H;
    return u;
}

// One launch shape for every form of k_project_count: a workgroup per segment of tc.seg records, stage[] as the form needs it.
// (segment-fed: stage[] first holds four waves' digit counters and the segment's reordered pairs, 24 KB — no more than the entries of a 1080p frame's segments need anyway)
template <class SRC, ProjLists LISTS, ProjKeys KEYS>
static hipError_t launch_segments(hipStream_t st, const SRC& src, size_t n, const PU& pu, const PreOut& out, const TileCount& tc) {
    size_t lds = LISTS == ProjLists::Stage ? (size_t)tc.scap * 8 : 0;
    if (KEYS == ProjKeys::SegmentFed) lds = std::max(lds, SEGFEED_LDS);
    if (WAVE_STORE<SRC>) lds = std::max(lds, wave_stages_at(KEYS == ProjKeys::SegmentFed) + WAVE_STAGES_BYTES);      // forms None and Count have no other use of stage[]
    k_project_count<SRC, LISTS, KEYS><<<dim3((unsigned)((n + tc.seg - 1) / tc.seg)), dim3(SEG_THREADS), lds, st>>>(src, (uint32_t)n, pu, out, tc);
    return hipGetLastError();
}
// fused key generation: the 4D sources alone (draw_common fuses a GS4D_MODE_4D_SORTED draw without quads, nothing else) — Src3D and Src2D have no such instance
template <class SRC> constexpr bool HAS_KEYS = !std::is_same<SRC, Src3D>::value && !std::is_same<SRC, Src2D>::value;
template <class SRC>
static hipError_t launch_pre(hipStream_t st, SRC src, size_t n, const Uniforms& un, int W, int H, PreOut out, const TileCount& tc) {
    if (n == 0) return hipSuccess;
    using L = ProjLists; using K = ProjKeys;
    const PU pu = make_pu(un, W, H);
    switch (tc.keys) {
    case K::None:
        switch (tc.lists) {
        case L::None: k_preprocess<SRC><<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st>>>(src, (uint32_t)n, pu, out, tc); return hipGetLastError();
        case L::Count: return launch_segments<SRC, L::Count, K::None>(st, src, n, pu, out, tc);
        case L::Stage: return launch_segments<SRC, L::Stage, K::None>(st, src, n, pu, out, tc);
        }
        break;
    case K::Write:
        if constexpr (HAS_KEYS<SRC>) switch (tc.lists) {
        case L::None: {
            // segments sized so that at most 2048 workgroups flush digit histograms (1024 global atomics each)
            TileCount t2 = tc;
            t2.seg = (uint32_t)std::max<size_t>(4096, (((n + 2047) / 2048) + SEG_THREADS - 1) / SEG_THREADS * SEG_THREADS);
            return launch_segments<SRC, L::None, K::Write>(st, src, n, pu, out, t2);
        }
        case L::Count: return launch_segments<SRC, L::Count, K::Write>(st, src, n, pu, out, tc);
        case L::Stage: return launch_segments<SRC, L::Stage, K::Write>(st, src, n, pu, out, tc);
        }
        break;
    case K::SegmentFed:
        if constexpr (HAS_KEYS<SRC>) if (tc.lists == L::Stage) return launch_segments<SRC, L::Stage, K::SegmentFed>(st, src, n, pu, out, tc);
        break;
    }
    return hipErrorInvalidValue;      // a pair the kernel has no instance for
}
hipError_t launch_preprocess_4d(hipStream_t st, const float4* soa, size_t soa_n, const SoaInfo& info, size_t n, const Uniforms& un, int W, int H, PreOut out, const TileCount& tc) {
    if (info.layout == SOA_STATIC3D) { Src4DStatic s{ soa, (uint32_t)soa_n, SoaConsts() }; for (int k = 0; k < 8; ++k) s.cs.v[k] = info.consts[k]; return launch_pre(st, s, n, un, W, H, out, tc); }
    return info.layout == SOA_SYM ? launch_pre(st, Src4DSym{ soa, (uint32_t)soa_n }, n, un, W, H, out, tc) : launch_pre(st, Src4D{ soa, (uint32_t)soa_n }, n, un, W, H, out, tc);
}
hipError_t launch_preprocess_3d(hipStream_t st, const float* verts72, size_t n, const Uniforms& un, int W, int H, PreOut out, const TileCount& tc) { return launch_pre(st, Src3D{ verts72 }, n, un, W, H, out, tc); }
hipError_t launch_preprocess_2d(hipStream_t st, const float* rec48, size_t n, const Uniforms& un, int W, int H, PreOut out, const TileCount& tc) { return launch_pre(st, Src2D{ rec48 }, n, un, W, H, out, tc); }

} // namespace gs4d
