// transform.hip — gs4d_transform_records (include/gs4d.h): the 96-byte records of a set under m 4D affine maps, x' = L x + o — mean
// L mu + o, covariance L Sigma L^T, colour copied — written as m * n records behind one another.
//
// One launch (more only past 2^22 workgroups), no workgroup ever waits for another:
//   k_transform_records  one workgroup of TRANSFORM_TILE threads per TRANSFORM_TILE source records and instance, in a one-dimensional grid: workgroup w
//                        is tile w % tiles of instance w / tiles.  The instance's gs4d_affine4 is uniform in the workgroup (the compiler reads it
//                        with scalar loads).  Thread r loads record r of the tile with six 16-byte loads — strided by 96 bytes across the lanes, but
//                        the six instructions of a wave use every byte of the lines they fetch — and evaluates it with the text of
//                        transform_record.h (this file is built with the flags of preprocess.hip: round to nearest, no contraction).  The output is
//                        what costs: a thread that stored its own record would put 16 of every 96 bytes on a line per store instruction.  The
//                        records are staged in LDS instead, six 16-byte pieces per record at a pitch of 7 pieces (odd, as in k_build_records: the
//                        lanes of a 16-byte LDS access fall on different slots of the bank row), and after one barrier the workgroup writes the
//                        tile's 6 * slots contiguous pieces with coalesced 16-byte stores.  GS4D_TRANSFORM_STAGED_LOAD (make lib
//                        TRANSFORM_STAGED_LOAD=1) stages the input the same way — coalesced loads of the tile's pieces into LDS, a barrier, every
//                        thread reading its record from its own slots: measured 2-11 % slower, never the shipped build.
// All byte offsets are 64-bit.  Of src only records < n are read, of xf only rows < m; of dst only records [0, m * n) behind the pointer given.
#include "gs4d_internal.h"
#include "transform_record.h"

namespace gs4d {

constexpr uint32_t TRANSFORM_THREADS = TRANSFORM_TILE;
constexpr uint32_t TRANSFORM_PIECES = 6;              // 16-byte pieces of a record
constexpr uint32_t TRANSFORM_PITCH = 7;               // pieces between two records in LDS
constexpr uint32_t TRANSFORM_MAX_GRID = 1u << 22;     // workgroups per launch: gridDim.x * blockDim.x stays below 2^32
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(TRANSFORM_THREADS) void k_transform_records(const f32x4* __restrict__ src, uint32_t n, uint32_t tiles,
                                                                         const gs4d_affine4* __restrict__ xf, uint32_t wg0, f32x4* __restrict__ dst) {
    __shared__ f32x4 stage[TRANSFORM_TILE * TRANSFORM_PITCH];
    const uint32_t wg = wg0 + blockIdx.x;                                                // (< tiles * m <= 0xFFFFFFFF: launch_transform_records)
    const uint32_t inst = wg / tiles;
    const uint64_t rec0 = (uint64_t)(wg - inst * tiles) * TRANSFORM_TILE;
    const uint64_t left = (uint64_t)n - rec0;                                            // (the grid has no workgroup past the end: left >= 1)
    const uint32_t slots = left < TRANSFORM_TILE ? (uint32_t)left : TRANSFORM_TILE;
    const uint32_t pieces = slots * TRANSFORM_PIECES;
    f32x4* const mine = stage + threadIdx.x * TRANSFORM_PITCH;
#ifdef GS4D_TRANSFORM_STAGED_LOAD
    {   // work item j of the tile is piece j % 6 of record j / 6, and the tile's pieces are contiguous in src
        const f32x4* const tile = src + rec0 * TRANSFORM_PIECES;
#pragma unroll
        for (uint32_t u = 0; u < TRANSFORM_PIECES; ++u) {
            const uint32_t j = threadIdx.x + u * TRANSFORM_THREADS;
            if (j < pieces) { const uint32_t r = j / TRANSFORM_PIECES; stage[r * TRANSFORM_PITCH + (j - r * TRANSFORM_PIECES)] = tile[j]; }
        }
    }
    __syncthreads();
#endif
    if (threadIdx.x < slots) {
#ifdef GS4D_TRANSFORM_STAGED_LOAD
        const f32x4* const rec = mine;                          // (nobody else reads or writes these slots before the barrier below)
#else
        const f32x4* const rec = src + (rec0 + threadIdx.x) * TRANSFORM_PIECES;
#endif
        float in[24], o[24];
#pragma unroll
        for (uint32_t k = 0; k < TRANSFORM_PIECES; ++k) { const f32x4 v = rec[k]; in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w; }
        const gs4d_affine4& a = xf[inst];
        gs4d_transform::record(a.l, a.o, in, o);
#pragma unroll
        for (uint32_t k = 0; k < TRANSFORM_PIECES; ++k) mine[k] = f32x4{ o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3] };
    }
    __syncthreads();
    f32x4* const tile = dst + ((uint64_t)inst * n + rec0) * TRANSFORM_PIECES;
#pragma unroll
    for (uint32_t u = 0; u < TRANSFORM_PIECES; ++u) {
        const uint32_t j = threadIdx.x + u * TRANSFORM_THREADS;
        if (j < pieces) { const uint32_t r = j / TRANSFORM_PIECES; tile[j] = stage[r * TRANSFORM_PITCH + (j - r * TRANSFORM_PIECES)]; }
    }
}

hipError_t launch_transform_records(hipStream_t st, const void* src, size_t n, const gs4d_affine4* xf, size_t m, void* dst) {
    if (!n || !m) return hipSuccess;
    const uint64_t tiles = (n + TRANSFORM_TILE - 1) / TRANSFORM_TILE, groups = tiles * m;
    if (n > 0xFFFFFFFFull || groups > 0xFFFFFFFFull) return hipErrorInvalidValue;        // (m * n <= 0xFFFFFFFF keeps tiles * m below that too)
    for (uint64_t g0 = 0; g0 < groups; g0 += TRANSFORM_MAX_GRID) {
        const uint64_t g = groups - g0 < TRANSFORM_MAX_GRID ? groups - g0 : TRANSFORM_MAX_GRID;
        k_transform_records<<<dim3((uint32_t)g), dim3(TRANSFORM_THREADS), 0, st>>>((const f32x4*)src, (uint32_t)n, (uint32_t)tiles, xf, (uint32_t)g0, (f32x4*)dst);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace gs4d
