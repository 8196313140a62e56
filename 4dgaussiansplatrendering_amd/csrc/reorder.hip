// reorder.hip — records in spatial order, and the gather that applies an index list to a record set (include/gs4d.h):
// gs4d_spatial_order (box, keys; the sort is sort.hip's) and gs4d_gather_records.
//
// Launches on one stream, no workgroup ever waits for another (kernel boundaries are the only dependencies):
//   k_order_box        up to RO_BOX_GROUPS workgroups walk the records with a grid stride: min and max of the three coordinates over the PLACED records
//                      (all three finite), reduced with wave shuffles, then across the waves in LDS — ONE partial of 6 floats per workgroup;
//   k_order_box_final  one workgroup: min / max of the partials -> box[6].  min and max of floats are exact, associative and commutative (no NaN
//                      reaches them; only the sign of a zero depends on the order, and it cannot change a cell: DESIGN.md §4), so the box does
//                      not depend on the grid, on the launch order or on which wave ran first;
//   k_order_keys       one thread per record: three strided float loads, the cell arithmetic of gs4d.h in float32 (this file is built with the
//                      flags of preprocess.hip: round to nearest, no contraction, correctly rounded division), the bit spread, one uint32 key;
//   k_gather_records   one workgroup per GATHER_TILE destination slots, copied in 16-byte pieces: dst is one contiguous, coalesced stream,
//                      the reads are the scattered side.  An entry >= nsrc leaves its slot alone.  All byte offsets are 64-bit.
#include "gs4d_internal.h"

namespace gs4d {

constexpr uint32_t RO_THREADS = 256, RO_WAVES = RO_THREADS / 64;
constexpr float RO_INF = __builtin_huge_valf();

__device__ __forceinline__ bool finite3(float x, float y, float z) { return fabsf(x) < RO_INF && fabsf(y) < RO_INF && fabsf(z) < RO_INF; }
__device__ __forceinline__ const float* record_pos(const char* __restrict__ src, uint64_t i, uint32_t stride, uint32_t pos_offset) {
    return (const float*)(src + i * stride + pos_offset);
}

// lo[0..2], hi[0..2] of the calling workgroup's threads -> out[6], written by thread 0
__device__ __forceinline__ void reduce_box(float (&lo)[3], float (&hi)[3], float* __restrict__ out) {
    __shared__ float part[RO_WAVES][6];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], d, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], d, 64)); }
    }
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { part[threadIdx.x >> 6][a] = lo[a]; part[threadIdx.x >> 6][3 + a] = hi[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6u) {
        float v = part[0][threadIdx.x];
        for (uint32_t w = 1; w < RO_WAVES; ++w) v = threadIdx.x < 3u ? fminf(v, part[w][threadIdx.x]) : fmaxf(v, part[w][threadIdx.x]);
        out[threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(RO_THREADS) void k_order_box(const char* __restrict__ src, uint32_t n, uint32_t stride, uint32_t pos_offset, float* __restrict__ partials) {
    float lo[3] = { RO_INF, RO_INF, RO_INF }, hi[3] = { -RO_INF, -RO_INF, -RO_INF };
    for (uint64_t i = (uint64_t)blockIdx.x * RO_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * RO_THREADS) {
        const float* p = record_pos(src, i, stride, pos_offset);
        const float x = p[0], y = p[1], z = p[2];
        if (finite3(x, y, z)) {
            lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
            hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
        }
    }
    reduce_box(lo, hi, partials + (size_t)blockIdx.x * 6);
}

__global__ __launch_bounds__(RO_THREADS) void k_order_box_final(const float* __restrict__ partials, uint32_t groups, float* __restrict__ box) {
    float lo[3] = { RO_INF, RO_INF, RO_INF }, hi[3] = { -RO_INF, -RO_INF, -RO_INF };
    for (uint32_t g = threadIdx.x; g < groups; g += RO_THREADS) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = fminf(lo[a], partials[(size_t)g * 6 + a]); hi[a] = fmaxf(hi[a], partials[(size_t)g * 6 + 3 + a]); }
    }
    reduce_box(lo, hi, box);
}

// 10 bits -> every third bit of 30
__device__ __forceinline__ uint32_t spread10(uint32_t v) {
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}
// gs4d.h: d = p - lo, e = hi - lo, g = (d / e) * 1023.0f; NaN (0 / 0, inf / inf) gives cell 0
__device__ __forceinline__ uint32_t order_cell(float p, float lo, float hi) {
    const float d = p - lo, e = hi - lo;
    const float g = (d / e) * 1023.0f;
    return g >= 0.0f ? (uint32_t)fminf(g, 1023.0f) : 0u;
}

__global__ __launch_bounds__(RO_THREADS) void k_order_keys(const char* __restrict__ src, uint32_t n, uint32_t stride, uint32_t pos_offset, const float* __restrict__ box, uint32_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * RO_THREADS + threadIdx.x;
    if (i >= n) return;
    const float* p = record_pos(src, i, stride, pos_offset);
    const float x = p[0], y = p[1], z = p[2];
    uint32_t key = ORDER_KEY_UNPLACED;
    if (finite3(x, y, z))
        key = spread10(order_cell(x, box[0], box[3])) | (spread10(order_cell(y, box[1], box[4])) << 1) | (spread10(order_cell(z, box[2], box[5])) << 2);
    keys[i] = key;
}

hipError_t launch_order_keys(hipStream_t st, const void* src, size_t n, size_t stride, size_t pos_offset, float* box_scratch, uint32_t* keys) {
    if (!n) return hipSuccess;
    const uint32_t groups = order_box_groups(n);
    float* const partials = box_scratch + 8;
    k_order_box<<<dim3(groups), dim3(RO_THREADS), 0, st>>>((const char*)src, (uint32_t)n, (uint32_t)stride, (uint32_t)pos_offset, partials);
    k_order_box_final<<<dim3(1), dim3(RO_THREADS), 0, st>>>(partials, groups, box_scratch);
    k_order_keys<<<dim3((uint32_t)((n + RO_THREADS - 1) / RO_THREADS)), dim3(RO_THREADS), 0, st>>>((const char*)src, (uint32_t)n, (uint32_t)stride, (uint32_t)pos_offset, box_scratch, keys);
    return hipGetLastError();
}

// ---- gs4d_gather_records ----
// The copy form of k_compact_scatter (compact.hip) with the list in memory instead of LDS: work item j of a tile moves piece j % q of the tile's
// slot j / q.  Four loads in flight per thread, issued unconditionally from a clamped address (an entry >= nsrc reads record 0; a work item past
// the end of the tile reads its last piece again), only the stores predicated: loads under the bounds test cost private memory.
constexpr uint32_t GATHER_TILE = 1024;          // destination slots per workgroup (<= 1024 * 64 pieces: 32-bit arithmetic within a tile)

__global__ __launch_bounds__(RO_THREADS) void k_gather_records(const uint32_t* __restrict__ index, uint64_t m, const uint4* __restrict__ src, uint32_t nsrc, uint32_t q, uint4* __restrict__ dst) {
    const uint64_t slot0 = (uint64_t)blockIdx.x * GATHER_TILE;
    const uint64_t left = m - slot0;                                                     // (the grid has no workgroup past the end: left >= 1)
    const uint32_t slots = left < GATHER_TILE ? (uint32_t)left : GATHER_TILE, pieces = slots * q;
    uint4* const out = dst + slot0 * q;
    for (uint32_t j0 = threadIdx.x; j0 < pieces; j0 += 4u * RO_THREADS) {
        uint32_t rec[4], piece[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t j = min(j0 + u * RO_THREADS, pieces - 1u);
            const uint32_t slot = j / q;
            piece[u] = j - slot * q;
            rec[u] = index[slot0 + slot];
        }
        uint4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) v[u] = src[(uint64_t)(rec[u] < nsrc ? rec[u] : 0u) * q + piece[u]];      // (nsrc >= 1: record 0 exists)
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) { const uint32_t j = j0 + u * RO_THREADS; if (j < pieces && rec[u] < nsrc) out[j] = v[u]; }
    }
}

// Rows of 4 or 8 bytes (a table of words, of gs4d_time_span): one row per work item, the same four unconditional loads and predicated stores.
template <class Row>
__global__ __launch_bounds__(RO_THREADS) void k_gather_rows(const uint32_t* __restrict__ index, uint64_t m, const Row* __restrict__ src, uint32_t nsrc, Row* __restrict__ dst) {
    const uint64_t j0 = (uint64_t)blockIdx.x * (4u * RO_THREADS) + threadIdx.x;
    uint32_t rec[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) { const uint64_t j = j0 + u * RO_THREADS; rec[u] = index[j < m ? j : m - 1u]; }      // (m >= 1)
    Row v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) v[u] = src[rec[u] < nsrc ? rec[u] : 0u];
#pragma unroll
    for (uint32_t u = 0; u < 4u; ++u) { const uint64_t j = j0 + u * RO_THREADS; if (j < m && rec[u] < nsrc) dst[j] = v[u]; }
}

hipError_t launch_gather_records(hipStream_t st, const uint32_t* index, size_t m, const void* src, size_t nsrc, size_t stride, void* dst) {
    if (!m || !nsrc) return hipSuccess;          // no entry can be < nsrc: every slot stays as it is
    const dim3 rows_grid((uint32_t)((m + 4 * RO_THREADS - 1) / (4 * RO_THREADS)));
    if (stride == 4) k_gather_rows<uint32_t><<<rows_grid, dim3(RO_THREADS), 0, st>>>(index, (uint64_t)m, (const uint32_t*)src, (uint32_t)nsrc, (uint32_t*)dst);
    else if (stride == 8) k_gather_rows<uint2><<<rows_grid, dim3(RO_THREADS), 0, st>>>(index, (uint64_t)m, (const uint2*)src, (uint32_t)nsrc, (uint2*)dst);
    else k_gather_records<<<dim3((uint32_t)((m + GATHER_TILE - 1) / GATHER_TILE)), dim3(RO_THREADS), 0, st>>>(index, (uint64_t)m, (const uint4*)src, (uint32_t)nsrc, (uint32_t)(stride / 16), (uint4*)dst);
    return hipGetLastError();
}

} // namespace gs4d
