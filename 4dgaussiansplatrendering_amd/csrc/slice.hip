// slice.hip — gs4d_slice_records (include/gs4d.h): the 96-byte records of a 4D set baked at one time — the conditional centre, the
// conditional covariance and the time opacity folded into alpha, with a time row and column that make a draw at mu_t_out a fixed point.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another:
//   k_slice_records  one workgroup of SLICE_TILE threads per SLICE_TILE records.  Thread r loads record r of the tile with six 16-byte loads and
//                    evaluates it with the text of slice_record.h (this file is built with the flags of preprocess.hip: round to nearest, no
//                    contraction, the same expf — word 7 is the alpha project_4d computes).  The records leave through the staged tile of
//                    record_tile.h.  Unlike gs4d_edit_colours and gs4d_shade_sh the kernel patches no shadow and reads none: the next draw
//                    repacks dst.
// All byte offsets are 64-bit.  Of src only records < n are read; of dst only records [0, n) behind the pointer given are written.
#include "gs4d_internal.h"
#include "slice_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t SLICE_THREADS = SLICE_TILE;

__global__ __launch_bounds__(SLICE_THREADS) void k_slice_records(const f32x4* __restrict__ src, uint32_t n, gs4d_slice q, uint32_t wg0, f32x4* __restrict__ dst) {
    __shared__ f32x4 stage[SLICE_TILE * RECORD_PITCH];
    const uint64_t rec0 = (uint64_t)(wg0 + blockIdx.x) * SLICE_TILE;                     // (< n <= 0xFFFFFFFF: launch_slice_records)
    const uint32_t slots = tile_slots((uint64_t)n - rec0, SLICE_TILE);                   // (the grid has no workgroup past the end: >= 1)
    if (threadIdx.x < slots) {
        float in[24], o[24];
        load_record(src + (rec0 + threadIdx.x) * RECORD_PIECES, in);
        gs4d_slicing::record(q.t, q.min_opacity, q.mu_t_out, q.s44_out, in, o);
        put_record(o, stage + threadIdx.x * RECORD_PITCH);
    }
    __syncthreads();
    store_staged<SLICE_THREADS>(dst + rec0 * RECORD_PIECES, stage, threadIdx.x, slots * RECORD_PIECES);
}

hipError_t launch_slice_records(hipStream_t st, const void* src, size_t n, const gs4d_slice& q, void* dst) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t groups = (n + SLICE_TILE - 1) / SLICE_TILE;
    return launch_runs(groups, [&](uint64_t g0, uint32_t g) {
        k_slice_records<<<dim3(g), dim3(SLICE_THREADS), 0, st>>>((const f32x4*)src, (uint32_t)n, q, (uint32_t)g0, (f32x4*)dst);
        return hipGetLastError();
    });
}

} // namespace gs4d
