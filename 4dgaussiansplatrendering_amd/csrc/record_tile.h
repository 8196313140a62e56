// record_tile.h — the one text of a tile of 96-byte records as the kernels that read or write whole records handle it (build.hip, transform.hip,
// transform_selected.hip, pose.hip, slice.hip), and of the host loop that launches them.  tests/record_tile_check.cpp compiles the
// plain part (everything outside __HIPCC__) with a CPU compiler.
//
// A thread that stored its own record would put 16 of every 96 bytes on a line per store instruction.  So thread r of a tile puts its record into
// LDS (put_record), and after a barrier the tile's 6 * slots pieces, which are contiguous in memory, are written with coalesced 16-byte stores
// (store_staged): work item `item` takes the pieces item, item + STEP, ... of the tile on its RECORD_PIECES turns, and piece j is piece j % 6 of
// record j / 6, at piece_slot(j) of the stage.  load_staged is the same walk from memory into the stage.
#ifndef GS4D_RECORD_TILE_H
#define GS4D_RECORD_TILE_H
#include <stdint.h>
#include "hd.h"

namespace gs4d {

constexpr uint32_t RECORD_PIECES = 6;                 // 16-byte pieces of a record
constexpr uint32_t RECORD_PITCH = 7;                  // pieces between two records in LDS.  Odd (as sh_pitch of shade.hip): the lanes of a 16-byte LDS
                                                      // access, a record apart, then fall on different slots of the bank row
constexpr uint32_t RECORD_MAX_GRID = 1u << 22;        // workgroups per launch: gridDim.x * blockDim.x stays below 2^32 at 256 threads

// the records of a tile of `tile` when `left` records remain from its first one: fewer only in the set's last tile
GS4D_HD inline uint32_t tile_slots(uint64_t left, uint32_t tile) { return left < tile ? (uint32_t)left : tile; }
// the piece of its tile that work item `item` takes on turn `turn` (< RECORD_PIECES), the items being `step` apart
GS4D_HD inline uint32_t turn_piece(uint32_t item, uint32_t turn, uint32_t step) { return item + turn * step; }
// where piece j of a tile stands in its stage: piece j % RECORD_PIECES of record j / RECORD_PIECES, the records RECORD_PITCH apart
GS4D_HD inline uint32_t piece_slot(uint32_t j) { const uint32_t r = j / RECORD_PIECES; return r * RECORD_PITCH + (j - r * RECORD_PIECES); }
// the workgroups that take `span` tiles between them, each `walk` of them a grid's width apart (pose.hip: t0 + blockIdx.x, + gridDim.x, ... below t1)
inline uint32_t walk_grid(uint32_t span, uint32_t walk) { return (span + walk - 1) / walk; }

// launch(g0, g) for the runs [g0, g0 + g) of at most max_grid that tile [0, groups), in order; the first result that is not Error{} (hipSuccess
// is 0) ends the walk and is returned
template <class Launch>
inline auto launch_runs(uint64_t groups, Launch launch, uint32_t max_grid = RECORD_MAX_GRID) -> decltype(launch((uint64_t)0, (uint32_t)0)) {
    typedef decltype(launch((uint64_t)0, (uint32_t)0)) Error;
    for (uint64_t g0 = 0; g0 < groups; ) {
        const uint32_t g = groups - g0 < max_grid ? (uint32_t)(groups - g0) : max_grid;
        const Error e = launch(g0, g);
        if (e != Error{}) return e;
        g0 += g;
    }
    return Error{};
}

#if defined(__HIPCC__)
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// the 24 floats of the record at rec: six 16-byte loads
__device__ __forceinline__ void load_record(const f32x4* rec, float in[24]) {
#pragma unroll
    for (uint32_t k = 0; k < RECORD_PIECES; ++k) { const f32x4 v = rec[k]; in[4 * k] = v.x; in[4 * k + 1] = v.y; in[4 * k + 2] = v.z; in[4 * k + 3] = v.w; }
}
// the 24 floats of a record to the six pieces at `to`: a thread's slots of the stage, or the record itself
__device__ __forceinline__ void put_record(const float o[24], f32x4* to) {
#pragma unroll
    for (uint32_t k = 0; k < RECORD_PIECES; ++k) to[k] = f32x4{ o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3] };
}

struct EveryRecord { __device__ bool operator()(uint32_t) const { return true; } };

// the first `pieces` pieces of a stage to the tile's pieces in memory, leaving out the records r of the tile for which !keep(r).  The work items
// are STEP apart: a workgroup's threads, or a wave's lanes
template <uint32_t STEP, class Keep = EveryRecord>
__device__ __forceinline__ void store_staged(f32x4* tile, const f32x4* stage, uint32_t item, uint32_t pieces, Keep keep = Keep()) {
#pragma unroll
    for (uint32_t u = 0; u < RECORD_PIECES; ++u) {
        const uint32_t j = turn_piece(item, u, STEP);
        if (j < pieces && keep(j / RECORD_PIECES)) tile[j] = stage[piece_slot(j)];
    }
}
// the tile's first `pieces` pieces in memory to their slots of a stage
template <uint32_t STEP>
__device__ __forceinline__ void load_staged(f32x4* stage, const f32x4* tile, uint32_t item, uint32_t pieces) {
#pragma unroll
    for (uint32_t u = 0; u < RECORD_PIECES; ++u) {
        const uint32_t j = turn_piece(item, u, STEP);
        if (j < pieces) stage[piece_slot(j)] = tile[j];
    }
}
#endif

} // namespace gs4d
#endif
