// edit.hip — gs4d_edit_colours (include/gs4d.h): the rgba of the selected records of a set edited in place — set, scaled, blended
// towards a colour or copied from another set — written into the records and, when the SoA shadow is current, into the shadow's colour plane.
//
// One launch, no workgroup ever waits for another, no LDS:
//   k_edit_colours<OP>  one workgroup per EDIT_TILE records, one record per thread.  A wave reads 1 KiB of consecutive table rows (one 16-byte load
//                       per thread, through keep_row: the predicate of gs4d_compact_records); a thread whose record is not selected is done.  A
//                       selected one loads the colour — from the shadow's plane 1 when that is being patched (it is current, so it holds the bits
//                       of floats 4..7 of the records; dense, fully coalesced), else from the 96-byte-strided records — and for COPY the colour of
//                       record i of `from`; edits the channels of the mask (this file is built with the flags of shade.hip: round to nearest, no
//                       contraction, every product and sum rounded on its own); and stores 16 bytes to the record and, if asked, 16 to the plane.
//                       The record store is 16 of every 96 bytes whatever is done: staging it would move the same partial lines.
// All byte offsets are 64-bit.  Nothing outside floats 4..7 of the selected records < n (and the same entries of the plane) is written; the table and
// `from` are only read, and only rows / records < n.
#include "gs4d_internal.h"

namespace gs4d {

template <int OP>
__global__ __launch_bounds__(EDIT_TILE) void k_edit_colours(float4* __restrict__ rec, uint32_t n, EditOp e, const uint4* __restrict__ stats, KeepRule k,
                                                            const float4* __restrict__ from, float4* plane1) {
    const uint64_t i = (uint64_t)blockIdx.x * EDIT_TILE + threadIdx.x;
    if (i >= n) return;
    if (stats && !keep_row(stats[i], k)) return;
    // (SET and COPY of all four channels need no old colour)
    const bool whole = (OP == GS4D_EDIT_SET || OP == GS4D_EDIT_COPY) && e.channels == 15u;
    float4 old = make_float4(0.0f, 0.0f, 0.0f, 0.0f), src = old;
    if (!whole) old = plane1 ? plane1[i] : rec[i * 6u + 1u];
    if (OP == GS4D_EDIT_COPY) src = from[i * 6u + 1u];
    float c[4] = { old.x, old.y, old.z, old.w };
    const float s[4] = { src.x, src.y, src.z, src.w };
#pragma unroll
    for (uint32_t ch = 0; ch < 4u; ++ch) {
        if (!((e.channels >> ch) & 1u)) continue;
        const float v = e.value[ch];
        if (OP == GS4D_EDIT_SET) c[ch] = v;
        else if (OP == GS4D_EDIT_MUL) c[ch] = c[ch] * v;
        else if (OP == GS4D_EDIT_LERP) c[ch] = c[ch] + (e.amount * (v - c[ch]));
        else c[ch] = s[ch];
    }
    const float4 out = make_float4(c[0], c[1], c[2], c[3]);
    rec[i * 6u + 1u] = out;
    if (plane1) plane1[i] = out;
}

hipError_t launch_edit_colours(hipStream_t st, void* records, size_t n, const EditOp& e, const gs4d_record_stat* stats, const KeepRule& rule,
                               const void* from, float4* plane1) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    if (!n) return hipSuccess;
    const dim3 grid((uint32_t)((n + EDIT_TILE - 1) / EDIT_TILE)), block(EDIT_TILE);
#define GS4D_EDIT(OP) k_edit_colours<OP><<<grid, block, 0, st>>>((float4*)records, (uint32_t)n, e, (const uint4*)stats, rule, (const float4*)from, plane1)
    switch (e.op) {
        case GS4D_EDIT_SET: GS4D_EDIT(GS4D_EDIT_SET); break;
        case GS4D_EDIT_MUL: GS4D_EDIT(GS4D_EDIT_MUL); break;
        case GS4D_EDIT_LERP: GS4D_EDIT(GS4D_EDIT_LERP); break;
        case GS4D_EDIT_COPY: GS4D_EDIT(GS4D_EDIT_COPY); break;
        default: return hipErrorInvalidValue;
    }
#undef GS4D_EDIT
    return hipGetLastError();
}

} // namespace gs4d
