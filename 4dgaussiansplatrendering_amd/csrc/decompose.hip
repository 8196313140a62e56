// decompose.hip — gs4d_decompose_records (include/gs4d.h): the splat parameters of a set of 96-byte records — position, orientation,
// scales, colour and, for a 4D set, a velocity with a temporal variance: gs4d_build_records backwards.
//
// One launch (more only past RECORD_MAX_GRID workgroups), no workgroup ever waits for another:
//   k_decompose_records<FORM, SOLVE>  one workgroup of DECOMPOSE_TILE threads per tile of DECOMPOSE_TILE records.  Thread r loads record r of the
//                                     tile with six 16-byte loads and evaluates it with the text of decompose_record.h (this file is built with
//                                     the flags of build.hip: round to nearest, no contraction, correctly rounded division and square root), then
//                                     stores its own rows: consecutive lanes write consecutive 16-, 12- and 4-byte rows, so every line written is
//                                     written whole and nothing is staged in LDS.  Which destinations are given is a uniform branch; SOLVE ==
//                                     false — neither rot nor scale is wanted — is the instance without the eigen-solve.  The matrix and the
//                                     eigenvectors live in registers: every index is a constant after unrolling, no instance uses scratch.
// All byte offsets are 64-bit.  Of src only records < n behind the pointer given are read; of every destination only rows < n are written.
#include "gs4d_internal.h"
#include "decompose_record.h"
#include "record_tile.h"

namespace gs4d {

constexpr uint32_t DECOMPOSE_THREADS = DECOMPOSE_TILE;
struct __attribute__((packed, aligned(4))) f32x3 { float x, y, z; };      // a 12-byte row: rows are 4-byte aligned only (build.hip)

template <int FORM, bool SOLVE>
__global__ __launch_bounds__(DECOMPOSE_THREADS) void k_decompose_records(const f32x4* __restrict__ src, uint32_t n, uint32_t t0, DecomposeOut o) {
    const uint64_t i = ((uint64_t)t0 + blockIdx.x) * DECOMPOSE_TILE + threadIdx.x;
    if (i >= n) return;
    float in[24];
    load_record(src + i * RECORD_PIECES, in);
    gs4d_decompose::Splat s;
    gs4d_decompose::record<FORM, SOLVE>(in, s);
    if (o.pos) {
        if (FORM == GS4D_PARAMS_3D) ((f32x3*)o.pos)[i] = f32x3{ s.pos[0], s.pos[1], s.pos[2] };
        else ((f32x4*)o.pos)[i] = f32x4{ s.pos[0], s.pos[1], s.pos[2], s.pos[3] };
    }
    if (o.rgba) ((f32x4*)o.rgba)[i] = f32x4{ s.rgba[0], s.rgba[1], s.rgba[2], s.rgba[3] };
    if (SOLVE) {
        if (o.rot) ((f32x4*)o.rot)[i] = f32x4{ s.q[0], s.q[1], s.q[2], s.q[3] };
        if (o.scale) ((f32x3*)o.scale)[i] = f32x3{ s.s[0], s.s[1], s.s[2] };
    }
    if (FORM != GS4D_PARAMS_3D) {
        if (o.dir) ((f32x3*)o.dir)[i] = f32x3{ s.dir[0], s.dir[1], s.dir[2] };
        if (o.tvar) ((float*)o.tvar)[i] = s.tvar;
    }
}

template <int FORM, bool SOLVE>
static hipError_t launch_instance(hipStream_t st, const void* src, uint32_t n, const DecomposeOut& o) {
    const uint32_t tiles = (uint32_t)(((uint64_t)n + DECOMPOSE_TILE - 1) / DECOMPOSE_TILE);      // (n <= 0xFFFFFFFF: tiles <= 2^24)
    return launch_runs(tiles, [&](uint64_t t0, uint32_t span) {
        k_decompose_records<FORM, SOLVE><<<dim3(span), dim3(DECOMPOSE_THREADS), 0, st>>>((const f32x4*)src, n, (uint32_t)t0, o);
        return hipGetLastError();
    });
}

hipError_t launch_decompose_records(hipStream_t st, int form, const void* src, size_t n, const DecomposeOut& o) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const bool solve = o.rot || o.scale;
    switch (form) {
        case GS4D_PARAMS_3D: return solve ? launch_instance<GS4D_PARAMS_3D, true>(st, src, (uint32_t)n, o) : launch_instance<GS4D_PARAMS_3D, false>(st, src, (uint32_t)n, o);
        case GS4D_PARAMS_4D_VEL: return solve ? launch_instance<GS4D_PARAMS_4D_VEL, true>(st, src, (uint32_t)n, o) : launch_instance<GS4D_PARAMS_4D_VEL, false>(st, src, (uint32_t)n, o);
        default: return hipErrorInvalidValue;
    }
}

} // namespace gs4d
