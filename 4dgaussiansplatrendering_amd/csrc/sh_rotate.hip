// sh_rotate.hip — gs4d_rotate_sh (include/gs4d.h): a rotated copy of a table of spherical-harmonic rows, every row under the rotation of
// the map that moves its record — map j of the call for every row (GS4D_SH_EACH, the instances of gs4d_transform_records), or the map its bind row
// chooses by the rules of gs4d_pose_records (GS4D_POSE_INDEX, GS4D_POSE_BLEND4) — or copied where it names no map or its map does not rotate.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another, no atomics:
//   k_rotate_sh<DEGREE, PATH>  one workgroup of T threads per tile of T rows (T = SHROT_TILE, SHROT_TILE_3 at degree 3, where a thread holds some 200
//                   registers), and with GS4D_SH_EACH per (tile, map).  Row traffic is that of k_shade_sh and record_tile.h:
//                   the used prefix of the tile's rows (Q = ceil(12 (DEGREE+1)^2 / 16) pieces of 16 bytes a row) is read with coalesced 16-byte
//                   loads, four in flight per thread, into LDS at a row pitch of Q | 1 pieces; thread r owns row r, reads it with 16-byte LDS reads,
//                   turns bands 1 .. DEGREE with the text of sh_rotate_record.h (this file is built with the flags of pose.hip: round to nearest,
//                   no contraction) and puts it back; after a barrier the prefix leaves with coalesced 16-byte stores.  A row that is copied is
//                   simply not touched in LDS, so its bytes — NaN payloads, the word behind 27 coefficients — are the source's.  The pieces behind
//                   the prefix go from load to store without LDS.  At degree 0 nothing is staged: the tile is one contiguous run of pieces.
//                   Every thread builds the frame and the matrices of its row's map in registers, band by band (D_3 after bands 1 and 2 are done
//                   with), for every PATH:
//                     EACH       the workgroup's one map, row `inst` of xf: the same address in every lane.
//                     INDEX      the row of xf that the thread's bind word names.
//                     BLEND4     the blended map of gs4d_pose::blend4.
//                   Matrices built once per workgroup into LDS — by thread 0 for EACH, by thread j < m for GS4D_POSE_INDEX with a small table — were
//                   built and measured, and did not pay: the workgroup waits at a barrier for a serial build that the redundant per-thread builds
//                   hide behind the row traffic (DESIGN.md §4 has the figures).
// All byte offsets are 64-bit.  Of src only rows < n are read, of bind only rows < n, of xf only rows < m; of dst only the rows the call names.
#include "gs4d_internal.h"
#include "sh_rotate_record.h"
#include "record_tile.h"

namespace gs4d {

enum : uint32_t { SHROT_PATH_EACH = 0, SHROT_PATH_INDEX = 1, SHROT_PATH_BLEND4 = 2 };

constexpr uint32_t SHROT_MAP_PIECES = 5;              // 16-byte pieces of a gs4d_affine4
constexpr uint32_t shrot_tile(int degree) { return degree >= 3 ? SHROT_TILE_3 : SHROT_TILE; }
constexpr uint32_t shrot_pieces(int degree) { return degree ? (12u * (uint32_t)gs4d_shrot::coeffs(degree) + 15u) / 16u : 0u; }      // 0, 3, 7, 12 (degree 0 stages nothing)
constexpr uint32_t shrot_pitch(int degree) { return shrot_pieces(degree) | 1u; }                                                  // 1, 3, 7, 13

// rows(j, r): the 20 floats of row j of the table in global memory, five 16-byte loads as written, because gs4d_pose::blend4 takes whole rows; the frame
// reads l[0..10] only, so pieces 3 and 4 are dead after inlining and it is left to the compiler to drop their loads
struct ShrotMaps {
    const f32x4* table;
    __device__ void operator()(uint32_t j, float r[20]) const {
        const f32x4* const p = table + (uint64_t)j * SHROT_MAP_PIECES;
#pragma unroll
        for (uint32_t k = 0; k < SHROT_MAP_PIECES; ++k) { const f32x4 v = p[k]; r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w; }
    }
};

// COUNT pieces from FIRST on of a thread's row in LDS, each one 16-byte read (the empty asm takes the piece whole, as in k_shade_sh)
template <uint32_t FIRST, uint32_t COUNT>
__device__ __forceinline__ void read_pieces(const f32x4* from, float* out) {
#pragma unroll
    for (uint32_t p = 0; p < COUNT; ++p) {
        f32x4 v = from[FIRST + p];
        asm volatile("" : "+v"(v));
        out[4 * p] = v.x; out[4 * p + 1] = v.y; out[4 * p + 2] = v.z; out[4 * p + 3] = v.w;
    }
}

template <int DEGREE, uint32_t PATH>
__global__ __launch_bounds__(shrot_tile(DEGREE)) void k_rotate_sh(const f32x4* __restrict__ src, uint32_t n, uint32_t row_pieces, const f32x4* __restrict__ xf,
                                                                   uint32_t m, const unsigned char* __restrict__ bind, uint64_t bind_stride, uint32_t inst0,
                                                                   uint32_t tile0, uint32_t tiles, f32x4* __restrict__ dst) {
    constexpr uint32_t TILE = shrot_tile(DEGREE), Q = shrot_pieces(DEGREE), P = shrot_pitch(DEGREE);
    __shared__ f32x4 rows[DEGREE ? TILE * P : 1];
    const uint32_t tid = threadIdx.x;
    // the tile, and with EACH the map: workgroup x of the run is tile x % tiles of instance inst0 + x / tiles (tile0 < tiles <= 2^25, blockIdx.x < 2^22)
    uint32_t t = tile0 + blockIdx.x, inst = 0;
    if (PATH == SHROT_PATH_EACH) { const uint32_t q = t / tiles; inst = inst0 + q; t -= q * tiles; }
    const uint64_t rec0 = (uint64_t)t * TILE;
    const uint32_t slots = tile_slots((uint64_t)n - rec0, TILE);                          // (t < tiles: >= 1)
    const f32x4* const in = src + rec0 * row_pieces;
    f32x4* const out = dst + ((uint64_t)inst * n + rec0) * row_pieces;
    if (DEGREE == 0) {
        // a row copy: the tile's rows are one run of slots * row_pieces pieces
        const uint32_t total = slots * row_pieces;
        for (uint32_t j0 = tid; j0 < total; j0 += 4u * TILE) {
            f32x4 v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) v[u] = in[min(j0 + u * TILE, total - 1u)];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) if (j0 + u * TILE < total) out[j0 + u * TILE] = v[u];
        }
        return;
    }
    // the bind row first: it travels while the table is staged (a thread past the end reads the tile's last row)
    const uint32_t r = tid < slots ? tid : slots - 1u;
    uint32_t j = 0;
    u32x4 jv = { 0, 0, 0, 0 };
    f32x4 wv = { 0, 0, 0, 0 };
    if (PATH == SHROT_PATH_EACH) j = inst;                                               // (inst < m)
    if (PATH == SHROT_PATH_INDEX) j = *(const uint32_t*)(bind + (rec0 + r) * bind_stride);
    if (PATH == SHROT_PATH_BLEND4) {
        const unsigned char* const row = bind + (rec0 + r) * bind_stride;
        jv = *(const u32x4*)row;
        wv = *(const f32x4*)(row + 16);
    }
    // the prefix: work item k of the tile is piece k % Q of row k / Q
    const uint32_t pieces = slots * Q;
    for (uint32_t k0 = tid; k0 < pieces; k0 += 4u * TILE) {
        uint32_t row[4], piece[4];
        f32x4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t k = min(k0 + u * TILE, pieces - 1u);
            row[u] = k / Q;
            piece[u] = k - row[u] * Q;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) v[u] = in[(uint64_t)row[u] * row_pieces + piece[u]];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) if (k0 + u * TILE < pieces) rows[row[u] * P + piece[u]] = v[u];
    }
    // behind the prefix: item k is piece Q + k % tail of row k / tail, the items TILE apart — (row, piece) is stepped, not divided
    const uint32_t tail = row_pieces - Q;
    if (tail) {
        const uint32_t dq = TILE / tail, dr = TILE - dq * tail;
        uint32_t row = tid / tail, piece = tid - row * tail;
        while (row < slots) {
            const uint64_t at = (uint64_t)row * row_pieces + Q + piece;
            out[at] = in[at];
            row += dq;
            piece += dr;
            if (piece >= tail) { piece -= tail; ++row; }
        }
    }
    __syncthreads();
    if (tid < slots) {
        f32x4* const mine = rows + tid * P;
        float c[Q ? 4 * Q : 4];
        bool turned = false;
        const ShrotMaps maps{ xf };
        float a[20];
        bool mapped;
        if (PATH == SHROT_PATH_BLEND4) {
            const unsigned int js[4] = { jv.x, jv.y, jv.z, jv.w };
            const float ws[4] = { wv.x, wv.y, wv.z, wv.w };
            mapped = gs4d_pose::blend4(maps, m, js, ws, a);
        } else {
            mapped = gs4d_shrot::index_map(maps, m, j, a);
        }
        if (mapped) {
            read_pieces<0, Q>(mine, c);
            turned = gs4d_shrot::coefficients<DEGREE>(a, c);
        }
        if (turned) {
#pragma unroll
            for (uint32_t p = 0; p < Q; ++p) mine[p] = f32x4{ c[4 * p], c[4 * p + 1], c[4 * p + 2], c[4 * p + 3] };
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < Q; ++u) {
        const uint32_t k = tid + u * TILE;
        if (k < pieces) { const uint32_t row = k / Q, piece = k - row * Q; out[(uint64_t)row * row_pieces + piece] = rows[row * P + piece]; }
    }
}

template <int DEGREE, uint32_t PATH>
static hipError_t launch_path(hipStream_t st, const void* src, uint32_t n, uint32_t row_pieces, const void* xf, uint32_t m, const void* bind, size_t bind_stride, void* dst) {
    constexpr uint32_t TILE = shrot_tile(DEGREE);
    const uint32_t tiles = (uint32_t)(((uint64_t)n + TILE - 1) / TILE);                  // (n <= 0xFFFFFFFF: tiles <= 2^25)
    const uint64_t groups = PATH == SHROT_PATH_EACH ? (uint64_t)tiles * m : tiles;       // (tile, map) pairs, the tiles of a map together
    return launch_runs(groups, [&](uint64_t g0, uint32_t span) {
        const uint32_t inst0 = PATH == SHROT_PATH_EACH ? (uint32_t)(g0 / tiles) : 0u, tile0 = PATH == SHROT_PATH_EACH ? (uint32_t)(g0 % tiles) : (uint32_t)g0;
        k_rotate_sh<DEGREE, PATH><<<dim3(span), dim3(TILE), 0, st>>>((const f32x4*)src, n, row_pieces, (const f32x4*)xf, m, (const unsigned char*)bind, (uint64_t)bind_stride,
                                                                     inst0, tile0, tiles, (f32x4*)dst);
        return hipGetLastError();
    });
}

template <int DEGREE>
static hipError_t launch_degree(hipStream_t st, const void* src, uint32_t n, uint32_t row_pieces, const void* xf, uint32_t m, const void* bind, uint32_t form,
                                size_t bind_stride, void* dst) {
    if (form == GS4D_SH_EACH) return launch_path<DEGREE, SHROT_PATH_EACH>(st, src, n, row_pieces, xf, m, bind, bind_stride, dst);
    if (form == GS4D_POSE_BLEND4) return launch_path<DEGREE, SHROT_PATH_BLEND4>(st, src, n, row_pieces, xf, m, bind, bind_stride, dst);
    if (form != GS4D_POSE_INDEX) return hipErrorInvalidValue;
    return launch_path<DEGREE, SHROT_PATH_INDEX>(st, src, n, row_pieces, xf, m, bind, bind_stride, dst);
}

hipError_t launch_rotate_sh(hipStream_t st, const void* src, size_t n, size_t stride, int degree, const gs4d_affine4* xf, size_t m, const void* bind, uint32_t form,
                            size_t bind_stride, void* dst) {
    if (!n || (form == GS4D_SH_EACH && !m)) return hipSuccess;
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || stride % 16 != 0 || stride < 16 || stride > 1024) return hipErrorInvalidValue;
    const uint32_t row_pieces = (uint32_t)(stride / 16);
    if (row_pieces < shrot_pieces(degree < 0 || degree > 3 ? 3 : degree)) return hipErrorInvalidValue;
    switch (degree) {
        case 0: return launch_degree<0>(st, src, (uint32_t)n, row_pieces, xf, (uint32_t)m, bind, form, bind_stride, dst);
        case 1: return launch_degree<1>(st, src, (uint32_t)n, row_pieces, xf, (uint32_t)m, bind, form, bind_stride, dst);
        case 2: return launch_degree<2>(st, src, (uint32_t)n, row_pieces, xf, (uint32_t)m, bind, form, bind_stride, dst);
        case 3: return launch_degree<3>(st, src, (uint32_t)n, row_pieces, xf, (uint32_t)m, bind, form, bind_stride, dst);
        default: return hipErrorInvalidValue;
    }
}

} // namespace gs4d
