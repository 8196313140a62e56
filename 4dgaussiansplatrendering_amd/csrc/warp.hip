// warp.hip — gs4d_warp_records (include/gs4d.h): every 96-byte record of a set pushed through the map x' = x + D(x) of a 4D lattice of
// displacement nodes, linearised at the record's own centre — mean mu + D(mu), covariance L Sigma L^T with L = I + grad D(mu) — or copied where the
// centre is not inside the lattice.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another:
//   k_warp_records  one workgroup of WARP_TILE threads per tile of WARP_TILE records.  Thread r loads record r of the tile with six 16-byte loads
//                   and evaluates it with the text of warp_record.h (this file is built with the flags of pose.hip: round to nearest, no
//                   contraction); the results — copied records too, so every tile is written whole — leave through the staged tile of
//                   record_tile.h.
//                   Two instances by the lattice's shape, both the one text: with a time axis a record gathers the 16 nodes of its cell, with
//                   dims[3] == 1 the 8 of its cube (an axis of one node has no level in the tree: fewer still for a sheet or a single node).
//                   What is particular is that gather, 128 or 256 bytes per record by a per-lane index against the 192 bytes streamed; the tree is
//                   walked depth first, so a pair of nodes is reduced as soon as it is there and no more than one part per level is live.
//                   Two builds were measured:
//                     nodes from global memory  the shipped build (WARP_LDS_NODES = 0): every thread loads its nodes with one 16-byte load each;
//                                               the lattice lives in the caches.  Two kernel instances.
//                     nodes from LDS            GS4D_WARP_LDS_NODES (make lib WARP_LDS_NODES=512): for a lattice of at most that many nodes the
//                                               workgroup copies it into LDS (coalesced 16-byte loads, from the L2 after the first workgroups) and
//                                               every thread reads its nodes from there; a larger lattice goes the way above.  The copy costs more
//                                               than the per-lane loads it replaces, which hit the L1 and the L2 anyway: never the shipped build.
//                                               GS4D_WARP_GLOBAL_LATTICE (make lib WARP_GLOBAL_LATTICE=1) takes the LDS way out of such a build again.
// All byte offsets are 64-bit.  Of src only records < n are read, of nodes only nodes < count (warp_record.h: whatever the records hold); of dst
// only records [0, n) behind the pointer given.
#include "gs4d_internal.h"
#include "warp_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t WARP_THREADS = WARP_TILE;
#if defined(GS4D_WARP_LDS_NODES) && !defined(GS4D_WARP_GLOBAL_LATTICE)
constexpr uint32_t LDS_CAPACITY = GS4D_WARP_LDS_NODES;        // nodes of the workgroup's LDS copy in the build that was measured against the shipped one
static_assert(LDS_CAPACITY <= 2048, "make lib WARP_LDS_NODES=<0..2048>: 32 KB beside the 28-KB stage");
#else
constexpr uint32_t LDS_CAPACITY = WARP_LDS_NODES;
#endif

// nodes(j, v): the four floats of node j of a lattice of 16-byte nodes, in global memory or in LDS
struct WarpNodes {
    const f32x4* lattice;
    __device__ void operator()(uint32_t j, float v[4]) const {
        const f32x4 d = lattice[j];                             // (j < count <= 2^28: the byte offset is 64-bit pointer arithmetic)
        v[0] = d.x; v[1] = d.y; v[2] = d.z; v[3] = d.w;
    }
};

template <bool TIME, bool LDS_NODES>
__global__ __launch_bounds__(WARP_THREADS) void k_warp_records(const f32x4* __restrict__ src, uint32_t n, const f32x4* __restrict__ nodes, uint32_t count,
                                                               const gs4d_lattice lat, uint32_t t0, f32x4* __restrict__ dst) {
    __shared__ f32x4 stage[WARP_TILE * RECORD_PITCH];
    __shared__ f32x4 lattice[LDS_NODES && LDS_CAPACITY ? LDS_CAPACITY : 1];
    if (LDS_NODES) {                                                                     // (count <= LDS_CAPACITY: launch_warp_records)
        for (uint32_t u = threadIdx.x; u < count; u += WARP_THREADS) lattice[u] = nodes[u];
        __syncthreads();
    }
    const WarpNodes fetch{ LDS_NODES ? lattice : nodes };
    const uint64_t rec0 = ((uint64_t)t0 + blockIdx.x) * WARP_TILE;
    const uint32_t slots = tile_slots((uint64_t)n - rec0, WARP_TILE);          // (the grid has no workgroup past the end: >= 1)
    f32x4* const mine = stage + threadIdx.x * RECORD_PITCH;
    if (threadIdx.x < slots) {
        float in[24], o[24];
        load_record(src + (rec0 + threadIdx.x) * RECORD_PIECES, in);
        gs4d_warp::record<TIME>(fetch, lat.lo, lat.inv, lat.dims, lat.clamp, in, o);
        put_record(o, mine);
    }
    __syncthreads();
    store_staged<WARP_THREADS>(dst + rec0 * RECORD_PIECES, stage, threadIdx.x, slots * RECORD_PIECES);
}

template <bool TIME, bool LDS_NODES>
static hipError_t launch_shape(hipStream_t st, const void* src, uint32_t n, const void* nodes, uint32_t count, const gs4d_lattice& lat, void* dst) {
    const uint32_t tiles = (uint32_t)(((uint64_t)n + WARP_TILE - 1) / WARP_TILE);        // (n <= 0xFFFFFFFF: tiles <= 2^24)
    return launch_runs(tiles, [&](uint64_t t0, uint32_t span) {
        k_warp_records<TIME, LDS_NODES><<<dim3(span), dim3(WARP_THREADS), 0, st>>>((const f32x4*)src, n, (const f32x4*)nodes, count, lat, (uint32_t)t0, (f32x4*)dst);
        return hipGetLastError();
    });
}

template <bool TIME>
static hipError_t launch_shape(hipStream_t st, const void* src, uint32_t n, const void* nodes, uint32_t count, const gs4d_lattice& lat, void* dst) {
    if constexpr (LDS_CAPACITY > 0) {                                                    // (the shipped build has no instance with the nodes in LDS)
        if (count <= LDS_CAPACITY) return launch_shape<TIME, true>(st, src, n, nodes, count, lat, dst);
    }
    return launch_shape<TIME, false>(st, src, n, nodes, count, lat, dst);
}

hipError_t launch_warp_records(hipStream_t st, const void* src, size_t n, const void* nodes, uint32_t count, const gs4d_lattice& lat, void* dst) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull || gs4d_warp::node_count(lat.dims, lat.clamp, lat.pad) != count) return hipErrorInvalidValue;
    if (lat.dims[3] >= 2u) return launch_shape<true>(st, src, (uint32_t)n, nodes, count, lat, dst);
    return launch_shape<false>(st, src, (uint32_t)n, nodes, count, lat, dst);
}

} // namespace gs4d
