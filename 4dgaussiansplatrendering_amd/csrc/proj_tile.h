// proj_tile.h — the one text of how a wave of k_project_count (preprocess.hip) hands its 64 projected records to memory, and of
// the LDS that takes.  tests/proj_tile_check.cpp compiles the plain part (everything outside __HIPCC__) with a CPU compiler.
//
// A projected record is one 64-byte line of four 16-byte pieces.  A thread that stored its own record would put 16 bytes on each of 64 lines per
// store instruction, and three more instructions would complete them.  So lane r of the wave puts its four pieces into the wave's stage in LDS
// (record_slot), and the wave's 4 * have pieces, which are contiguous in memory, leave with whole-line stores: a lane takes the pieces lane, lane + 64,
// ... of the wave (turn_piece) on its PROJ_PIECES turns, and piece j is piece j % 4 of record j / 4, at piece_slot(j) of the stage.
#ifndef GS4D_PROJ_TILE_H
#define GS4D_PROJ_TILE_H
#include <stdint.h>
#include "hd.h"

namespace gs4d {
namespace proj_tile {

constexpr uint32_t WAVE = 64;                         // records of a wave's round: one per lane
constexpr uint32_t PIECES = 4;                        // 16-byte pieces of a projected record
constexpr uint32_t PITCH_DENSE = 4, PITCH_ODD = 5;    // pieces between two records in LDS: the records back to back, or — as RECORD_PITCH of record_tile.h —
                                                      // an odd number of pieces apart, so that the lanes of a put fall on different slots of the bank row
#if defined(GS4D_PROJ_PITCH)
constexpr uint32_t PITCH = GS4D_PROJ_PITCH;           // make lib PROJ_PITCH=4: the measurement of DESIGN.md §9 round 16; never the shipped build
#else
constexpr uint32_t PITCH = PITCH_ODD;
#endif
static_assert(PITCH >= PIECES, "the records of a stage do not overlap");

// the records of the wave whose first record is `first` that lie below `end`: 0 for a wave at or past the end
GS4D_HD inline uint32_t wave_have(uint32_t first, uint32_t end) { return first >= end ? 0u : end - first < WAVE ? end - first : WAVE; }
// where the record of lane r stands in the wave's stage, in pieces: it fills [record_slot(r), record_slot(r) + PIECES)
GS4D_HD inline uint32_t record_slot(uint32_t r, uint32_t pitch) { return r * pitch; }
// the piece of the wave's range that `lane` takes on turn `turn` (< PIECES)
GS4D_HD inline uint32_t turn_piece(uint32_t lane, uint32_t turn) { return lane + turn * WAVE; }
// where piece j of the wave's range stands in the stage: piece j % PIECES of record j / PIECES
GS4D_HD inline uint32_t piece_slot(uint32_t j, uint32_t pitch) { return record_slot(j / PIECES, pitch) + j % PIECES; }
// bytes of `waves` stages
GS4D_HD constexpr uint32_t stage_bytes(uint32_t waves, uint32_t pitch) { return waves * WAVE * pitch * 16u; }

#if defined(__HIPCC__)
// Only the wave's own lanes read what a lane puts: a wave's LDS instructions execute in order, so nothing has to wait — the fence and the barrier
// keep the compiler from moving an LDS access of one side to the other.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
// lane r's record into the wave's stage (Piece: a 16-byte type)
template <class Piece>
__device__ __forceinline__ void put_record(Piece* stage, uint32_t r, const Piece (&o)[PIECES]) {
    static_assert(sizeof(Piece) == 16, "a piece is 16 bytes");
#pragma unroll
    for (uint32_t k = 0; k < PIECES; ++k) stage[record_slot(r, PITCH) + k] = o[k];
}
// the stage's first PIECES * have pieces to the wave's range of the record array, `to` being the wave's first record there.  Called by all 64 lanes,
// behind a wave_sync() that follows the puts; no address at or beyond piece PIECES * have is formed.
template <class Piece>
__device__ __forceinline__ void store_staged(Piece* to, const Piece* stage, uint32_t lane, uint32_t have) {
#pragma unroll
    for (uint32_t t = 0; t < PIECES; ++t) {
        const uint32_t j = turn_piece(lane, t);
        if (j < PIECES * have) to[j] = stage[piece_slot(j, PITCH)];
    }
}
#endif

} // namespace proj_tile
} // namespace gs4d
#endif
