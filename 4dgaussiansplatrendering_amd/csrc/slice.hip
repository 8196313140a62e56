// slice.hip — gs4d_slice_records (include/gs4d.h): the 96-byte records of a 4D set baked at one time — the conditional centre, the
// conditional covariance and the time opacity folded into alpha, with a time row and column that make a draw at mu_t_out a fixed point.
//
// One launch (more only past 2^22 workgroups), no workgroup ever waits for another:
//   k_slice_records  the shape of k_transform_records: one workgroup of SLICE_TILE threads per SLICE_TILE records.  Thread r loads record r of the
//                    tile with six 16-byte loads and evaluates it with the text of slice_record.h (this file is built with the flags of
//                    preprocess.hip: round to nearest, no contraction, the same expf — word 7 is the alpha project_4d computes).  The records are
//                    staged in LDS, six 16-byte pieces per record at a pitch of 7 pieces, and after one barrier the workgroup writes the tile's
//                    6 * slots contiguous pieces with coalesced 16-byte stores.  Unlike gs4d_edit_colours and gs4d_shade_sh the kernel patches no
//                    shadow and reads none: the next draw repacks dst.
// All byte offsets are 64-bit.  Of src only records < n are read; of dst only records [0, n) behind the pointer given are written.
#include "gs4d_internal.h"
#include "slice_record.h"

namespace gs4d {

constexpr uint32_t SLICE_THREADS = SLICE_TILE;
constexpr uint32_t SLICE_PIECES = 6;              // 16-byte pieces of a record
constexpr uint32_t SLICE_PITCH = 7;               // pieces between two records in LDS
constexpr uint32_t SLICE_MAX_GRID = 1u << 22;     // workgroups per launch: gridDim.x * blockDim.x stays below 2^32
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(SLICE_THREADS) void k_slice_records(const f32x4* __restrict__ src, uint32_t n, gs4d_slice q, uint32_t wg0, f32x4* __restrict__ dst) {
    __shared__ f32x4 stage[SLICE_TILE * SLICE_PITCH];
    const uint64_t rec0 = (uint64_t)(wg0 + blockIdx.x) * SLICE_TILE;                     // (< n <= 0xFFFFFFFF: launch_slice_records)
    const uint64_t left = (uint64_t)n - rec0;                                            // (the grid has no workgroup past the end: left >= 1)
    const uint32_t slots = left < SLICE_TILE ? (uint32_t)left : SLICE_TILE;
    const uint32_t pieces = slots * SLICE_PIECES;
    f32x4* const mine = stage + threadIdx.x * SLICE_PITCH;
    if (threadIdx.x < slots) {
        const f32x4* const rec = src + (rec0 + threadIdx.x) * SLICE_PIECES;
        float in[24], o[24];
#pragma unroll
        for (uint32_t k = 0; k < SLICE_PIECES; ++k) { const f32x4 v = rec[k]; in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w; }
        gs4d_slicing::record(q.t, q.min_opacity, q.mu_t_out, q.s44_out, in, o);
#pragma unroll
        for (uint32_t k = 0; k < SLICE_PIECES; ++k) mine[k] = f32x4{ o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3] };
    }
    __syncthreads();
    f32x4* const tile = dst + rec0 * SLICE_PIECES;
#pragma unroll
    for (uint32_t u = 0; u < SLICE_PIECES; ++u) {
        const uint32_t j = threadIdx.x + u * SLICE_THREADS;
        if (j < pieces) { const uint32_t r = j / SLICE_PIECES; tile[j] = stage[r * SLICE_PITCH + (j - r * SLICE_PIECES)]; }
    }
}

hipError_t launch_slice_records(hipStream_t st, const void* src, size_t n, const gs4d_slice& q, void* dst) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t groups = (n + SLICE_TILE - 1) / SLICE_TILE;
    for (uint64_t g0 = 0; g0 < groups; g0 += SLICE_MAX_GRID) {
        const uint64_t g = groups - g0 < SLICE_MAX_GRID ? groups - g0 : SLICE_MAX_GRID;
        k_slice_records<<<dim3((uint32_t)g), dim3(SLICE_THREADS), 0, st>>>((const f32x4*)src, (uint32_t)n, q, (uint32_t)g0, (f32x4*)dst);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

} // namespace gs4d
