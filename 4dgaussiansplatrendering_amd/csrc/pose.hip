// pose.hip — gs4d_pose_records (include/gs4d.h): every 96-byte record of a set under the map ITS bind row chooses among the m rows of
// a gs4d_affine4 table — one row by index (GS4D_POSE_INDEX) or up to four rows blended by weight (GS4D_POSE_BLEND4) — or copied where the row names
// no row of the table.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another:
//   k_pose_records  one workgroup of POSE_TILE threads per tile of POSE_TILE records; it takes the tiles t0 + blockIdx.x, + gridDim.x, ... below t1.
//                   Thread r loads record r of the tile with six 16-byte loads and evaluates it with the text of pose_record.h (this file is
//                   built with the flags of preprocess.hip: round to nearest, no contraction); the results — copied records too, so every tile
//                   is written whole — leave through the staged tile of record_tile.h.  The bind row is one 4-byte load (INDEX) or two 16-byte
//                   loads (BLEND4) per thread.
//                   What is particular is the gather of the table rows, 80 bytes per row and up to four rows per record, by a per-lane index.
//                   Three builds were measured:
//                     rows from LDS, one tile   the shipped build: for m <= POSE_LDS_ROWS the workgroup copies the table into LDS (coalesced
//                                               16-byte loads, from the L2 after the first workgroups) and every thread reads its rows from
//                                               there; a larger table goes the way below.  One tile per workgroup.
//                     rows from global memory   GS4D_POSE_GLOBAL_TABLE (make lib POSE_GLOBAL_TABLE=1): every thread loads its rows with five
//                                               16-byte loads each for every m; the table lives in the caches.  One tile per workgroup.
//                     rows from LDS, a walk     GS4D_POSE_WALK (make lib POSE_WALK=4): as the first, but a workgroup takes POSE_WALK tiles, a
//                                               grid's width apart, so that its copy of the table is paid once per POSE_WALK * POSE_TILE records.
//                                               The copy turned out to be cheap and the walk dear: never the shipped build.
// All byte offsets are 64-bit.  Of src only records < n are read, of bind only rows < n, of xf only rows < m; of dst only records [0, n) behind the
// pointer given.
#include "gs4d_internal.h"
#include "pose_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t POSE_THREADS = POSE_TILE;
constexpr uint32_t POSE_ROW_PIECES = 5;               // 16-byte pieces of a gs4d_affine4
#ifndef GS4D_POSE_WALK
#define GS4D_POSE_WALK 1
#endif
constexpr uint32_t POSE_WALK = GS4D_POSE_WALK;        // tiles a workgroup with the table in LDS takes
static_assert(POSE_WALK >= 1 && POSE_WALK <= 64, "make lib POSE_WALK=<1..64>");

// rows(j, r): the 20 floats of row j of a table of 16-byte pieces, in global memory or in LDS
struct PoseRows {
    const f32x4* table;
    __device__ void operator()(uint32_t j, float r[20]) const {
        const f32x4* const p = table + (uint64_t)j * POSE_ROW_PIECES;
#pragma unroll
        for (uint32_t k = 0; k < POSE_ROW_PIECES; ++k) { const f32x4 v = p[k]; r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w; }
    }
};

template <uint32_t FORM, bool LDS_TABLE>
__global__ __launch_bounds__(POSE_THREADS) void k_pose_records(const f32x4* __restrict__ src, uint32_t n, const f32x4* __restrict__ xf, uint32_t m,
                                                               const unsigned char* __restrict__ bind, uint64_t bind_stride, uint32_t t0, uint32_t t1,
                                                               f32x4* __restrict__ dst) {
    __shared__ f32x4 stage[POSE_TILE * RECORD_PITCH];
    __shared__ f32x4 table[LDS_TABLE ? POSE_LDS_ROWS * POSE_ROW_PIECES : 1];
    if (LDS_TABLE) {                                                                     // (m <= POSE_LDS_ROWS: launch_pose_records)
        for (uint32_t u = threadIdx.x; u < m * POSE_ROW_PIECES; u += POSE_THREADS) table[u] = xf[u];
        __syncthreads();
    }
    const PoseRows rows{ LDS_TABLE ? table : xf };
    f32x4* const mine = stage + threadIdx.x * RECORD_PITCH;
    for (uint64_t t = (uint64_t)t0 + blockIdx.x; t < t1; t += gridDim.x) {               // (uniform in the workgroup: every thread meets every barrier)
        const uint64_t rec0 = t * POSE_TILE;
        const uint32_t slots = tile_slots((uint64_t)n - rec0, POSE_TILE);     // (t < t1 <= tiles: >= 1)
        if (threadIdx.x < slots) {
            const uint64_t i = rec0 + threadIdx.x;
            const f32x4* const rec = src + i * RECORD_PIECES;
            const unsigned char* const row = bind + i * bind_stride;
            float in[24], o[24];
            load_record(rec, in);
            if (FORM == GS4D_POSE_INDEX) {
                gs4d_pose::index(rows, m, *(const uint32_t*)row, in, o);
            } else {
                const u32x4 jv = *(const u32x4*)row;
                const f32x4 wv = *(const f32x4*)(row + 16);
                const unsigned int j[4] = { jv.x, jv.y, jv.z, jv.w };
                const float w[4] = { wv.x, wv.y, wv.z, wv.w };
                gs4d_pose::blend(rows, m, j, w, in, o);
            }
            put_record(o, mine);
        }
        __syncthreads();
        // store_staged<POSE_THREADS> of record_tile.h, spelled out.  Here the walk stands in a loop, its slot arithmetic is moved in front of the
        // loop, and with the call the compiler puts it in front of the kernel's argument loads too: every wave then starts some 30
        // instructions later
        f32x4* const tile = dst + rec0 * RECORD_PIECES;
        const uint32_t pieces = slots * RECORD_PIECES;
#pragma unroll
        for (uint32_t u = 0; u < RECORD_PIECES; ++u) {
            const uint32_t j = threadIdx.x + u * POSE_THREADS;
            if (j < pieces) { const uint32_t r = j / RECORD_PIECES; tile[j] = stage[r * RECORD_PITCH + (j - r * RECORD_PIECES)]; }
        }
        __syncthreads();                                                            // the next tile's records are staged over these
    }
}

template <uint32_t FORM, bool LDS_TABLE>
static hipError_t launch_form(hipStream_t st, const void* src, uint32_t n, const void* xf, uint32_t m, const void* bind, size_t bind_stride, void* dst) {
    constexpr uint32_t walk = LDS_TABLE ? POSE_WALK : 1u;                                // tiles per workgroup
    const uint32_t tiles = (uint32_t)(((uint64_t)n + POSE_TILE - 1) / POSE_TILE);        // (n <= 0xFFFFFFFF: tiles <= 2^24)
    return launch_runs(tiles, [&](uint64_t t0, uint32_t span) {                          // spans of tiles: walk of them to a workgroup
        k_pose_records<FORM, LDS_TABLE><<<dim3(walk_grid(span, walk)), dim3(POSE_THREADS), 0, st>>>((const f32x4*)src, n, (const f32x4*)xf, m, (const unsigned char*)bind,
                                                                                                    (uint64_t)bind_stride, (uint32_t)t0, (uint32_t)t0 + span, (f32x4*)dst);
        return hipGetLastError();
    }, RECORD_MAX_GRID * walk);
}

template <uint32_t FORM>
static hipError_t launch_form(hipStream_t st, const void* src, uint32_t n, const void* xf, uint32_t m, const void* bind, size_t bind_stride, void* dst) {
#ifndef GS4D_POSE_GLOBAL_TABLE
    if (m <= POSE_LDS_ROWS) return launch_form<FORM, true>(st, src, n, xf, m, bind, bind_stride, dst);
#endif
    return launch_form<FORM, false>(st, src, n, xf, m, bind, bind_stride, dst);
}

hipError_t launch_pose_records(hipStream_t st, const void* src, size_t n, const gs4d_affine4* xf, size_t m, const void* bind, uint32_t form,
                               size_t bind_stride, void* dst) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (form == GS4D_POSE_INDEX) return launch_form<GS4D_POSE_INDEX>(st, src, (uint32_t)n, xf, (uint32_t)m, bind, bind_stride, dst);
    if (form == GS4D_POSE_BLEND4) return launch_form<GS4D_POSE_BLEND4>(st, src, (uint32_t)n, xf, (uint32_t)m, bind, bind_stride, dst);
    return hipErrorInvalidValue;
}

} // namespace gs4d
