// transform.hip — gs4d_transform_records (include/gs4d.h): the 96-byte records of a set under m 4D affine maps, x' = L x + o — mean
// L mu + o, covariance L Sigma L^T, colour copied — written as m * n records behind one another.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another:
//   k_transform_records  one workgroup of TRANSFORM_TILE threads per TRANSFORM_TILE source records and instance, in a one-dimensional grid: workgroup w
//                        is tile w % tiles of instance w / tiles.  The instance's gs4d_affine4 is uniform in the workgroup (the compiler reads it
//                        with scalar loads).  Thread r loads record r of the tile with six 16-byte loads — strided by 96 bytes across the lanes, but
//                        the six instructions of a wave use every byte of the lines they fetch — and evaluates it with the text of
//                        transform_record.h (this file is built with the flags of preprocess.hip: round to nearest, no contraction).  The records
//                        leave through the staged tile of record_tile.h.  GS4D_TRANSFORM_STAGED_LOAD (make lib TRANSFORM_STAGED_LOAD=1) stages the
//                        input the same way — coalesced loads of the tile's pieces into LDS, a barrier, every thread reading its record from its
//                        own slots: measured 2-11 % slower, never the shipped build.
// All byte offsets are 64-bit.  Of src only records < n are read, of xf only rows < m; of dst only records [0, m * n) behind the pointer given.
#include "gs4d_internal.h"
#include "transform_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t TRANSFORM_THREADS = TRANSFORM_TILE;

__global__ __launch_bounds__(TRANSFORM_THREADS) void k_transform_records(const f32x4* __restrict__ src, uint32_t n, uint32_t tiles,
                                                                         const gs4d_affine4* __restrict__ xf, uint32_t wg0, f32x4* __restrict__ dst) {
    __shared__ f32x4 stage[TRANSFORM_TILE * RECORD_PITCH];
    const uint32_t wg = wg0 + blockIdx.x;                                                // (< tiles * m <= 0xFFFFFFFF: launch_transform_records)
    const uint32_t inst = wg / tiles;
    const uint64_t rec0 = (uint64_t)(wg - inst * tiles) * TRANSFORM_TILE;
    const uint32_t slots = tile_slots((uint64_t)n - rec0, TRANSFORM_TILE);     // (the grid has no workgroup past the end: >= 1)
    const uint32_t pieces = slots * RECORD_PIECES;
    f32x4* const mine = stage + threadIdx.x * RECORD_PITCH;
#ifdef GS4D_TRANSFORM_STAGED_LOAD
    load_staged<TRANSFORM_THREADS>(stage, src + rec0 * RECORD_PIECES, threadIdx.x, pieces);
    __syncthreads();
#endif
    if (threadIdx.x < slots) {
#ifdef GS4D_TRANSFORM_STAGED_LOAD
        const f32x4* const rec = mine;                          // (nobody else reads or writes these slots before the barrier below)
#else
        const f32x4* const rec = src + (rec0 + threadIdx.x) * RECORD_PIECES;
#endif
        float in[24], o[24];
        load_record(rec, in);
        const gs4d_affine4& a = xf[inst];
        gs4d_transform::record(a.l, a.o, in, o);
        put_record(o, mine);
    }
    __syncthreads();
    store_staged<TRANSFORM_THREADS>(dst + ((uint64_t)inst * n + rec0) * RECORD_PIECES, stage, threadIdx.x, pieces);
}

hipError_t launch_transform_records(hipStream_t st, const void* src, size_t n, const gs4d_affine4* xf, size_t m, void* dst) {
    if (!n || !m) return hipSuccess;
    const uint64_t tiles = (n + TRANSFORM_TILE - 1) / TRANSFORM_TILE, groups = tiles * m;
    if (n > 0xFFFFFFFFull || groups > 0xFFFFFFFFull) return hipErrorInvalidValue;        // (m * n <= 0xFFFFFFFF keeps tiles * m below that too)
    return launch_runs(groups, [&](uint64_t g0, uint32_t g) {
        k_transform_records<<<dim3(g), dim3(TRANSFORM_THREADS), 0, st>>>((const f32x4*)src, (uint32_t)n, (uint32_t)tiles, xf, (uint32_t)g0, (f32x4*)dst);
        return hipGetLastError();
    });
}

} // namespace gs4d
