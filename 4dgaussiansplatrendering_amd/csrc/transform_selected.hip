// transform_selected.hip — gs4d_transform_selected (include/gs4d.h): the selected ones of the 96-byte records of a set moved in place
// under one 4D affine map about a pivot — mean L (mu - c) + o + c, covariance L Sigma L^T, colour copied — the pivot given, or taken on the device
// from the 96 bytes of a gs4d_measure.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another and no wave waits for another — there is no barrier:
//   k_transform_selected  one workgroup of XFSEL_TILE threads per XFSEL_TILE records, each wave on its own 64 of them.  Thread r loads row r of the
//                         tile's table rows first (one 16-byte load, 1 KiB of consecutive rows per wave, through keep_row: the predicate of
//                         gs4d_edit_colours); the ballot of the wave's selected lanes is its selected mask, uniform in the wave.  A wave in which
//                         nothing is selected ends there: it has read 16 bytes per record and writes nothing.  A thread whose record is not
//                         selected loads nothing else.  A selected one loads its record with six 16-byte loads and evaluates the text of
//                         transform_record.h (this file is built with the flags of transform.hip: round to nearest, no contraction).  The map
//                         and the pivot are kernel arguments, uniform; with GS4D_XS_PIVOT_MEASURE the pivot is gs4d_transform::measure_centre
//                         of the measurement, read with uniform loads and evaluated in double by the waves that hold a selected record — the
//                         same value in every lane, no launch of its own.
//                         A wave with at least XFSEL_STAGE_MIN selected records stages them in its own quarter of the LDS array — the
//                         staged tile of record_tile.h, a wave's 64 records wide — and then walks the 6 * 64 contiguous pieces of its records,
//                         leaving out the pieces of records whose bit in the selected mask is clear: a run of selected records is written as
//                         whole lines, and a record that is not selected is never touched.  The LDS operations of one wave execute in order,
//                         so the wave needs no barrier between staging and walking — only a wavefront-scope fence, which keeps the compiler
//                         from moving the reads up.  A wave with fewer selected records lets each of them store its own six pieces: the
//                         walk's six masked store instructions and the LDS round trip cost more than the few partial lines (the threshold is
//                         measured: DESIGN.md §4).  GS4D_XFSEL_PLAIN (make lib XFSEL_PLAIN=1) is the plain form throughout — no LDS: the
//                         measurement of DESIGN.md §4, never the shipped build.
// All byte offsets are 64-bit.  Threads past n neither load nor store; of stats only rows < n are read, of measure its first 96 bytes; of data only
// the selected records < n are read and written.
#include "gs4d_internal.h"
#include "transform_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t XFSEL_THREADS = XFSEL_TILE;
constexpr uint32_t XFSEL_WAVE = 64;
#ifndef GS4D_XFSEL_STAGE_MIN
#define GS4D_XFSEL_STAGE_MIN 8
#endif
constexpr uint32_t XFSEL_STAGE_MIN = GS4D_XFSEL_STAGE_MIN;      // selected records of a wave from which it stages its stores
static_assert(XFSEL_TILE % XFSEL_WAVE == 0, "whole waves");

// the record at rec under x about its pivot, to `to` (the record itself, or its slots in LDS)
__device__ __forceinline__ void move_record(const f32x4* rec, const gs4d_selection_xf& x, const gs4d_measure* __restrict__ measure, f32x4* to) {
    const bool pivot = x.flags != 0u;                                                    // (GS4D_XS_PIVOT or GS4D_XS_PIVOT_MEASURE: validated)
    float c[3] = { x.pivot[0], x.pivot[1], x.pivot[2] };
    if (x.flags == (uint32_t)GS4D_XS_PIVOT_MEASURE) gs4d_transform::measure_centre(measure->count, measure->lo, measure->hi, (const unsigned long long*)measure->cell_sum, c);
    float in[24], o[24];
    load_record(rec, in);
    gs4d_transform::record_about(x.xf.l, x.xf.o, pivot, c, in, o);
    put_record(o, to);
}

__global__ __launch_bounds__(XFSEL_THREADS) void k_transform_selected(f32x4* data, uint32_t n, gs4d_selection_xf x, const uint4* __restrict__ stats, KeepRule k,
                                                                      const gs4d_measure* __restrict__ measure, uint32_t wg0) {
    const uint64_t rec0 = (uint64_t)(wg0 + blockIdx.x) * XFSEL_TILE;                     // (< n <= 0xFFFFFFFF: launch_transform_selected)
    const uint32_t slots = tile_slots((uint64_t)n - rec0, XFSEL_TILE);                   // (the grid has no workgroup past the end: >= 1)
    const bool selected = threadIdx.x < slots && (!stats || keep_row(stats[rec0 + threadIdx.x], k));
    const uint64_t mask = __ballot(selected);                                            // the wave's selected records, bit = lane
    if (mask == 0ull) return;
    f32x4* const rec = data + (rec0 + threadIdx.x) * RECORD_PIECES;
#ifndef GS4D_XFSEL_PLAIN
    if ((uint32_t)__popcll(mask) >= XFSEL_STAGE_MIN) {                                   // (uniform in the wave)
        __shared__ f32x4 stage[XFSEL_TILE * RECORD_PITCH];
        const uint32_t lane = threadIdx.x & (XFSEL_WAVE - 1u), first = threadIdx.x - lane;      // first: the wave's first record of the tile (< slots: mask != 0)
        f32x4* const mine = stage + first * RECORD_PITCH;                                // this wave's quarter; no other wave reads or writes it
        if (selected) move_record(rec, x, measure, mine + lane * RECORD_PITCH);
        // (the wave's LDS writes are performed before its LDS reads below: one wave's LDS operations execute in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // the wave's records are a tile of their own, XFSEL_WAVE wide, that begins at record `first` of the workgroup's
        store_staged<XFSEL_WAVE>(data + (rec0 + first) * RECORD_PIECES, mine, lane, tile_slots(slots - first, XFSEL_WAVE) * RECORD_PIECES,
                                 [mask](uint32_t r) { return ((mask >> r) & 1ull) != 0ull; });
        return;
    }
#endif
    if (selected) move_record(rec, x, measure, rec);
}

hipError_t launch_transform_selected(hipStream_t st, void* data, size_t n, const gs4d_selection_xf& xf, const gs4d_record_stat* stats, const KeepRule& rule,
                                     const gs4d_measure* measure) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (xf.flags == (uint32_t)GS4D_XS_PIVOT_MEASURE ? !measure : xf.flags > (uint32_t)GS4D_XS_PIVOT) return hipErrorInvalidValue;
    const uint64_t groups = (n + XFSEL_TILE - 1) / XFSEL_TILE;
    return launch_runs(groups, [&](uint64_t g0, uint32_t g) {
        k_transform_selected<<<dim3(g), dim3(XFSEL_THREADS), 0, st>>>((f32x4*)data, (uint32_t)n, xf, (const uint4*)stats, rule, measure, (uint32_t)g0);
        return hipGetLastError();
    });
}

} // namespace gs4d
