// centres.hip — gs4d_count_centres (include/gs4d.h): the records of a set whose time-conditioned centre lies in a volume and / or
// projects into a region of the screen, as rows of a record-statistics table.  The predicate is the text of centre_query.h, which the host definition
// compiles too; this file is built with the flags of shade.hip (round to nearest, no contraction, every product and sum rounded on its own).
//
// One launch, no LDS, no workgroup ever waits for another:
//   k_count_centres<SRC, COL>  one workgroup per CENTRES_TILE records, one record per thread.  A thread loads what the definition reads of its record —
//                       SRC == CQ_RECORDS: the 16-byte pieces 0 (position, mu_t) and 5 (sig[3]) of the 96-byte record; otherwise the record buffer's SoA
//                       shadow, which the host has found current and which holds the same bits: plane 0 and the sig[3] plane (CQ_PLANES: the full and the
//                       symmetric layout, which differ only in where that plane lies; dense, fully coalesced, 32 bytes a record), or plane 0 and five
//                       kernel arguments (CQ_STATIC: 16 bytes a record) — and, COL only (GS4D_CQ_SKIP_HIDDEN), the colour piece / plane for the alpha.
//                       The test flags are run-time branches, uniform over the launch.  A mask byte is one 1-byte load at the pixel the centre falls on.
//   the row update      add_fragments: a plain 16-byte load, modify, store by the one thread that owns row i.  No atomics: the call takes the table as a kernel write
//                       that keeps the contents (queue_on_lane's "out", gs4d_api.hip) — the draws that add to it are settled before the launch and every
//                       later adder, reader and the host order themselves behind it — so nothing else touches the table while the kernel runs, and
//                       within the kernel row i belongs to thread i alone.  Rows of records that do not take part are neither read nor written.
// All byte offsets are 64-bit.  Nothing but rows < n of the table is written; records, shadow and mask are only read, and only records < n and mask
// bytes inside the query's rectangle.
#include "gs4d_internal.h"
#include "centre_query.h"

namespace gs4d {

enum { CQ_RECORDS = 0, CQ_PLANES = 1, CQ_STATIC = 2 };
// where the fields come from.  CQ_RECORDS: rec.  The others: pos = plane 0, col = plane 1, sig3 = the sig[3] plane (soa_sig3; CQ_STATIC: null, and
// mu_t, sig[3] are cmut, csig3 for every record)
struct CentreSrc { const float4* rec; const float4* pos; const float4* col; const float4* sig3; float4 csig3; float cmut; };

template <int SRC, bool COL>
__global__ __launch_bounds__(CENTRES_TILE) void k_count_centres(CentreSrc s, uint32_t n, gs4d_centre_query q, float hw, float hh, const uint8_t* __restrict__ mask,
                                                                uint4* __restrict__ stats) {
    const uint64_t i = (uint64_t)blockIdx.x * CENTRES_TILE + threadIdx.x;
    if (i >= n) return;
    float4 p, g;
    float alpha = 0.0f;
    if (SRC == CQ_RECORDS) {
        p = s.rec[i * 6u];
        g = s.rec[i * 6u + 5u];
        if (COL) alpha = s.rec[i * 6u + 1u].w;
    } else {
        p = s.pos[i];
        if (SRC == CQ_STATIC) { g = s.csig3; p.w = s.cmut; }      // (plane 0 of this layout carries sig[0][0] in .w)
        else g = s.sig3[i];
        if (COL) alpha = s.col[i].w;
    }
    const gs4d_centre::Fields r{ { p.x, p.y, p.z }, p.w, alpha, { g.x, g.y, g.z }, g.w };
    if (!gs4d_centre::takes_part(q, hw, hh, r, mask)) return;
    if (q.op == (uint32_t)GS4D_CQ_ADD) add_fragments(stats, i, 1u, WEIGHT_ONE_BITS);
    else stats[i] = make_uint4(0u, 0u, 0u, 0u);
}

hipError_t launch_count_centres(hipStream_t st, const void* records, const float4* soa, size_t soa_n, const SoaInfo& info, size_t n, const gs4d_centre_query& q,
                                int W, int H, const uint8_t* mask, gs4d_record_stat* stats) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    static_assert(sizeof(gs4d_centre_query) == 256, "the query travels as a kernel argument");
    if (!n) return hipSuccess;
    const dim3 grid((uint32_t)((n + CENTRES_TILE - 1) / CENTRES_TILE)), block(CENTRES_TILE);
    const float hw = (float)W * 0.5f, hh = (float)H * 0.5f;
    const bool col = (q.tests & (uint32_t)GS4D_CQ_SKIP_HIDDEN) != 0u;
    CentreSrc s{ (const float4*)records, soa, soa ? soa + soa_n : nullptr, soa ? soa_sig3(soa, soa_n, info) : nullptr,
                 make_float4(info.consts[4], info.consts[5], info.consts[6], info.consts[7]), info.consts[0] };
    const int src = !soa ? CQ_RECORDS : info.layout == SOA_STATIC3D ? CQ_STATIC : CQ_PLANES;
#define GS4D_CENTRES(SRC) do { if (col) k_count_centres<SRC, true><<<grid, block, 0, st>>>(s, (uint32_t)n, q, hw, hh, mask, (uint4*)stats); \
                               else k_count_centres<SRC, false><<<grid, block, 0, st>>>(s, (uint32_t)n, q, hw, hh, mask, (uint4*)stats); } while (0)
    switch (src) {
        case CQ_RECORDS: GS4D_CENTRES(CQ_RECORDS); break;
        case CQ_PLANES: GS4D_CENTRES(CQ_PLANES); break;
        default: GS4D_CENTRES(CQ_STATIC); break;
    }
#undef GS4D_CENTRES
    return hipGetLastError();
}

} // namespace gs4d
