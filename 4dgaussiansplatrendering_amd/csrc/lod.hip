// lod.hip — gs4d_lod_append and gs4d_lod_cut (include/gs4d.h): a forest of merged levels assembled on the device, and the cut a
// camera and a time make through it.  The predicate is the text of lod_query.h, which the host definition compiles too; this file is built with the
// flags of shade.hip (round to nearest, no contraction, every product and sum rounded on its own).
//
// gs4d_lod_append is one launch (k_lod_append), one thread per item: the 6 m 16-byte pieces of the level's records, copied as they are, then the m
// parent words of the new nodes (GS4D_ID_NONE), then the c parent words of the children.  The words are 4-byte stores: `first` and `child_first`
// are any node index, so a run of words has no 16-byte alignment to rely on.
//
// gs4d_lod_cut, on one stream; no workgroup ever waits for another (kernel boundaries are the only dependencies):
//   k_lod_clear    one thread: the caller's gs4d_lod_count <- {0, 0, 0, 0};
//   k_lod_levels   one launch per level from the top down (a run of consecutive levels that fit one tile together: ONE launch of one workgroup, a
//                  __syncthreads() between two levels).  One workgroup per LOD_TILE nodes of the level, LOD_ROUNDS nodes per thread, LOD_THREADS
//                  apart: a wave reads 256 consecutive bytes of parent words.  A thread loads its parent words (coalesced), gathers the state byte
//                  of every parent that is one (a root has none), and only a round in which some lane of the WAVE is tested goes on: its tested
//                  lanes load pieces 0, 2, 3, 4 and 5 of their record (16 bytes each; a leaf loads nothing: tested, it is drawn), evaluate `fine`
//                  and — stats — add one fragment to their own row (add_fragments).  Every thread stores its node's state byte.  STOP path: 4 bytes
//                  of parent, 1 gathered, 1 stored.  tested and drawn_leaves are popcounts of wave ballots, summed over the rounds in a wave-uniform
//                  register; lane 0 of each wave leaves its pair in LDS (32 bytes: the only LDS of the kernel), and thread 0 adds the workgroup's
//                  pair with ONE 64-bit atomic on words 2 and 3 of the count (tested low, drawn_leaves high: tested <= n < 2^32 never carries) —
//                  none where the workgroup tested nothing;
//   the compaction k_compact_count / k_compact_scan / k_compact_scatter over the state plane (compact.hip, Row = uint8_t, the rule "is DRAW"): the
//                  DRAW nodes in ascending index into dst and cut_index, under the capacity, and words 0 and 1 of the count.
// Scratch (the lane's): the state plane of n bytes, and compact_tiles(n) words.  Every byte of the plane is written before it is read: every node
// lies in exactly one level, and a parent word is followed only where it names a higher level, whose launch is over.  All byte offsets are 64-bit.
// nodes and parent are only read, and only rows < n; a parent's state is read only for p < n.
#include "gs4d_internal.h"
#include "lod_query.h"
#include "record_tile.h"      // f32x4

namespace gs4d {

namespace lod = gs4d_lod;
constexpr uint32_t LOD_THREADS = 256, LOD_WAVES = LOD_THREADS / 64, LOD_ROUNDS = LOD_TILE / LOD_THREADS;
static_assert(LOD_TILE % LOD_THREADS == 0 && LOD_ROUNDS >= 1, "whole rounds");
static_assert(sizeof(gs4d_lod_count) == sizeof(uint4) && sizeof(gs4d_lod_query) == 112 && offsetof(gs4d_lod_count, tested) == 8, "the structures of gs4d.h");

// ---- gs4d_lod_append ----
__global__ __launch_bounds__(LOD_THREADS) void k_lod_append(const uint4* __restrict__ level, uint64_t m, const uint32_t* __restrict__ member_group, uint64_t c,
                                                            uint4* __restrict__ nodes_at_first, uint32_t* __restrict__ parent, uint32_t first, uint32_t child_first) {
    const uint64_t w = (uint64_t)blockIdx.x * LOD_THREADS + threadIdx.x;
    if (w < 6u * m) { nodes_at_first[w] = level[w]; return; }
    if (w < 7u * m) { parent[(uint64_t)first + (w - 6u * m)] = GS4D_ID_NONE; return; }
    const uint64_t i = w - 7u * m;
    if (i >= c) return;
    const uint32_t g = member_group[i];
    parent[(uint64_t)child_first + i] = g < m ? first + g : GS4D_ID_NONE;      // (first + m <= 0xFFFFFFFE: no wrap)
}

hipError_t launch_lod_append(hipStream_t st, const void* level, size_t m, const uint32_t* member_group, size_t child_first, size_t c,
                             void* nodes, uint32_t* parent, size_t first) {
    const uint64_t items = 7ull * m + c;
    if (!items) return hipSuccess;
    if (first + m > 0xFFFFFFFEull || child_first + c > first) return hipErrorInvalidValue;
    k_lod_append<<<dim3((uint32_t)((items + LOD_THREADS - 1) / LOD_THREADS)), dim3(LOD_THREADS), 0, st>>>(
        (const uint4*)level, (uint64_t)m, member_group, (uint64_t)c, (uint4*)((char*)nodes + first * 96), parent, (uint32_t)first, (uint32_t)child_first);
    return hipGetLastError();
}

// ---- gs4d_lod_cut ----
struct LodLevels { uint32_t first[17]; };      // gs4d_lod_query::level_first, as a kernel argument

__global__ void k_lod_clear(uint4* __restrict__ count) { *count = make_uint4(0u, 0u, 0u, 0u); }

// levels k_hi down to k_lo; more than one level: ONE workgroup, and every level of the run fits its tile
__global__ __launch_bounds__(LOD_THREADS) void k_lod_levels(const f32x4* __restrict__ nodes, const uint32_t* __restrict__ parent, uint8_t* __restrict__ state,
                                                            uint32_t n, LodLevels lv, int k_hi, int k_lo, lod::View view, uint4* __restrict__ stats,
                                                            unsigned long long* __restrict__ counters) {
    __shared__ uint2 wave_pair[LOD_WAVES];
    uint32_t tested_sum = 0u, leaves_sum = 0u;                 // wave-uniform
    for (int k = k_hi; k >= k_lo; --k) {
        const uint32_t end = lv.first[k + 1];
        const uint64_t tile0 = (uint64_t)lv.first[k] + (uint64_t)blockIdx.x * LOD_TILE;
        const bool leaf = k == 0;
        uint32_t p[LOD_ROUNDS];
        uint8_t ps[LOD_ROUNDS];
#pragma unroll
        for (uint32_t r = 0; r < LOD_ROUNDS; ++r) {
            const uint64_t i = tile0 + r * LOD_THREADS + threadIdx.x;
            p[r] = i < end ? parent[i] : GS4D_ID_NONE;
        }
#pragma unroll
        for (uint32_t r = 0; r < LOD_ROUNDS; ++r) {
            const uint64_t i = tile0 + r * LOD_THREADS + threadIdx.x;
            ps[r] = i < end && lod::is_child(p[r], end, n) ? state[p[r]] : (uint8_t)lod::DESCEND;      // a root is tested
        }
#pragma unroll
        for (uint32_t r = 0; r < LOD_ROUNDS; ++r) {
            const uint64_t i = tile0 + r * LOD_THREADS + threadIdx.x;
            const bool in = i < end, test = in && ps[r] == lod::DESCEND;
            const uint64_t mask = __ballot(test);
            uint8_t s = lod::STOP;
            if (mask != 0ull) {                                 // (wave-uniform) else: no record of this round is looked at
                if (test) {
                    bool is_fine = false;
                    if (!leaf) {
                        const f32x4* const rec = nodes + i * 6u;
                        const f32x4 a = rec[0], c2 = rec[2], c3 = rec[3], c4 = rec[4], g = rec[5];
                        const gs4d_centre::Fields f{ { a.x, a.y, a.z }, a.w, 0.0f, { g.x, g.y, g.z }, g.w };
                        is_fine = lod::fine(view, f, c2.x, c3.y, c4.z);
                    }
                    s = lod::tested_state(leaf, is_fine);
                    if (s == lod::DRAW && stats) add_fragments(stats, i, 1u, WEIGHT_ONE_BITS);
                }
                const uint32_t c = (uint32_t)__popcll(mask);
                tested_sum += c;
                if (leaf) leaves_sum += c;                      // a tested leaf is drawn
            }
            if (in) state[i] = s;
        }
        if (k > k_lo) __syncthreads();                          // (one workgroup) the states of level k are what level k - 1 gathers
    }
    if ((threadIdx.x & 63u) == 0u) wave_pair[threadIdx.x >> 6] = make_uint2(tested_sum, leaves_sum);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0u, l = 0u;
        for (uint32_t w = 0; w < LOD_WAVES; ++w) { t += wave_pair[w].x; l += wave_pair[w].y; }
        if (t != 0u) atomicAdd(counters, (unsigned long long)t | ((unsigned long long)l << 32));
    }
}

hipError_t launch_lod_cut(hipStream_t st, const void* nodes, const uint32_t* parent, size_t n, const gs4d_lod_query& q, uint8_t* state,
                          uint32_t* tile_counts, void* dst, uint32_t* cut_index, gs4d_record_stat* stats, uint32_t cap, gs4d_lod_count* count) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    if (!lod::query_ok(q, n)) return hipErrorInvalidValue;
    k_lod_clear<<<dim3(1), dim3(1), 0, st>>>((uint4*)count);
    if (!n) return hipGetLastError();
    LodLevels lv;
    for (int k = 0; k < 17; ++k) lv.first[k] = k <= (int)q.levels ? q.level_first[k] : (uint32_t)n;
    const lod::View view = lod::view_of(q);
    unsigned long long* const counters = (unsigned long long*)&count->tested;      // words 2 and 3: 8-byte aligned in a device allocation
    auto size = [&](int k) { return (uint64_t)(lv.first[k + 1] - lv.first[k]); };
    for (int k = (int)q.levels - 1; k >= 0;) {
        int lo = k;
        uint64_t total = size(k);
        uint32_t groups;
        if (total <= LOD_TILE) {                                // the run of levels below it that fit one tile with it
            while (lo > 0 && total + size(lo - 1) <= LOD_TILE) total += size(--lo);
            groups = total ? 1u : 0u;
        } else groups = (uint32_t)((total + LOD_TILE - 1) / LOD_TILE);
        if (groups)
            k_lod_levels<<<dim3(groups), dim3(LOD_THREADS), 0, st>>>((const f32x4*)nodes, parent, state, (uint32_t)n, lv, k, lo, view, (uint4*)stats, counters);
        k = lo - 1;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_compact(st, state, n, DrawRule{ lod::DRAW }, tile_counts, nodes, 96, dst, cut_index, cap, (gs4d_compact_count*)count);
}

} // namespace gs4d
