// build.hip — gs4d_build_records (include/gs4d.h): the 96-byte records of a splat set from its parameters — position, orientation,
// scales, colour and, for a 4D set, a velocity with a temporal variance or a second rotation.
//
// One launch, no workgroup ever waits for another:
//   k_build_records<FORM>  one workgroup of BUILD_TILE threads per BUILD_TILE records.  Thread r of the workgroup owns record r of the tile: it loads
//                          its rows — a 16-byte row with one 16-byte load, a 12-byte row with one 12-byte load; consecutive lanes read consecutive
//                          rows, so every fetched line is used — and evaluates the record with the text of build_record.h (this file is built with
//                          the flags of preprocess.hip: round to nearest, no contraction, correctly rounded division and square root).  The records
//                          leave through the staged tile of record_tile.h.  GS4D_BUILD_PLAIN (make lib BUILD_PLAIN=1) leaves the staging out, every
//                          thread storing its own record: the measurement of DESIGN.md §4, never the shipped build.
// All byte offsets are 64-bit.  Of the parameters only rows < n are read; of dst only records < n are written.
#include "gs4d_internal.h"
#include "build_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t BUILD_THREADS = BUILD_TILE;
struct __attribute__((packed, aligned(4))) f32x3 { float x, y, z; };      // a 12-byte row: rows are 4-byte aligned only

template <int FORM>
__global__ __launch_bounds__(BUILD_THREADS) void k_build_records(BuildParams p, uint32_t n, f32x4* __restrict__ dst) {
#ifndef GS4D_BUILD_PLAIN
    __shared__ f32x4 stage[BUILD_TILE * RECORD_PITCH];
#endif
    const uint64_t rec0 = (uint64_t)blockIdx.x * BUILD_TILE;
    const uint32_t slots = tile_slots((uint64_t)n - rec0, BUILD_TILE);     // (the grid has no workgroup past the end: >= 1)
    if (threadIdx.x < slots) {
        const uint64_t i = rec0 + threadIdx.x;
        const f32x4 q = ((const f32x4*)p.rot)[i], col = ((const f32x4*)p.rgba)[i];
        float o[24];
        if (FORM == GS4D_PARAMS_3D) {
            const f32x3 ps = ((const f32x3*)p.pos)[i], sc = ((const f32x3*)p.scale)[i];
            const float pos[3] = { ps.x, ps.y, ps.z }, s[3] = { sc.x, sc.y, sc.z }, qq[4] = { q.x, q.y, q.z, q.w }, c[4] = { col.x, col.y, col.z, col.w };
            gs4d_build::record_3d(pos, qq, s, c, o);
        } else if (FORM == GS4D_PARAMS_4D_VEL) {
            const f32x4 ps = ((const f32x4*)p.pos)[i];
            const f32x3 sc = ((const f32x3*)p.scale)[i], d = ((const f32x3*)p.dir)[i];
            const float sd = ((const float*)p.tvar)[i];
            const float pos[4] = { ps.x, ps.y, ps.z, ps.w }, s[3] = { sc.x, sc.y, sc.z }, dir[3] = { d.x, d.y, d.z };
            const float qq[4] = { q.x, q.y, q.z, q.w }, c[4] = { col.x, col.y, col.z, col.w };
            gs4d_build::record_4d_vel(pos, qq, s, dir, sd, c, o);
        } else {
            const f32x4 ps = ((const f32x4*)p.pos)[i], qr = ((const f32x4*)p.rot_r)[i], sc = ((const f32x4*)p.scale)[i];
            const float pos[4] = { ps.x, ps.y, ps.z, ps.w }, s[4] = { sc.x, sc.y, sc.z, sc.w }, q1[4] = { qr.x, qr.y, qr.z, qr.w };
            const float qq[4] = { q.x, q.y, q.z, q.w }, c[4] = { col.x, col.y, col.z, col.w };
            gs4d_build::record_4d_2q(pos, qq, q1, s, c, o);
        }
#ifdef GS4D_BUILD_PLAIN
        put_record(o, dst + i * RECORD_PIECES);
#else
        put_record(o, stage + threadIdx.x * RECORD_PITCH);
#endif
    }
#ifndef GS4D_BUILD_PLAIN
    __syncthreads();
    store_staged<BUILD_THREADS>(dst + rec0 * RECORD_PIECES, stage, threadIdx.x, slots * RECORD_PIECES);
#endif
}

hipError_t launch_build_records(hipStream_t st, int form, const BuildParams& p, size_t n, void* dst) {
    if (!n) return hipSuccess;
    const uint64_t groups = ((uint64_t)n + BUILD_TILE - 1) / BUILD_TILE;
    if (groups * BUILD_THREADS > 0xFFFFFFFFull) return hipErrorInvalidValue;             // one grid: gridDim.x * blockDim.x stays below 2^32
    const dim3 grid((uint32_t)groups), block(BUILD_THREADS);
    switch (form) {
        case GS4D_PARAMS_3D: k_build_records<GS4D_PARAMS_3D><<<grid, block, 0, st>>>(p, (uint32_t)n, (f32x4*)dst); break;
        case GS4D_PARAMS_4D_VEL: k_build_records<GS4D_PARAMS_4D_VEL><<<grid, block, 0, st>>>(p, (uint32_t)n, (f32x4*)dst); break;
        case GS4D_PARAMS_4D_2Q: k_build_records<GS4D_PARAMS_4D_2Q><<<grid, block, 0, st>>>(p, (uint32_t)n, (f32x4*)dst); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

} // namespace gs4d
