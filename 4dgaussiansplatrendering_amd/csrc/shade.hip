// shade.hip — gs4d_shade_sh (include/gs4d.h): the colour of every record from its row of spherical-harmonic coefficients, for one
// camera position and one time, written into the records and — when the SoA shadow is current — into the shadow's colour plane.
//
// One launch, no workgroup ever waits for another:
//   k_shade_sh<DEGREE>  one workgroup per SHADE_TILE records.  The cost is the table: the used prefix of the tile's rows (Q = ceil(12 (DEGREE+1)^2 / 16)
//                       pieces of 16 bytes per row) is read with coalesced 16-byte loads, four in flight per thread, issued unconditionally from a
//                       clamped address as in k_gather_records (reorder.hip), and written to LDS with a row pitch of Q | 1 pieces: an odd pitch
//                       puts the 16 lanes of every group of a 16-byte LDS read on 16 different slots of the bank row, so the per-record reads that
//                       follow are conflict-free.  Thread r of the workgroup then owns record r of the tile: two 16-byte loads from the record
//                       (floats 0..3 and 20..23, issued before the table is staged), the direction, the basis and the three sums in the order
//                       gs4d.h fixes (this file is built with the flags of preprocess.hip: round to nearest, no contraction, correctly rounded
//                       division and square root), and three floats stored to the record and, if asked, to the shadow's plane 1.
// All byte offsets are 64-bit.  Nothing outside floats 4..6 of records < n (and .xyz of the same entries of the plane) is written; of the table
// only the first 16 Q bytes of rows < n are read.
#include "gs4d_internal.h"
#include "record_tile.h"      // f32x4

namespace gs4d {

constexpr uint32_t SH_THREADS = SHADE_TILE;
constexpr float SH_INF = __builtin_huge_valf();

// the constants of the 3DGS reference implementation (computeColorFromSH), rounded to float32
constexpr float SH_C0 = 0.28209479177387814f, SH_C1 = 0.4886025119029199f;
constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_1 = -1.0925484305920792f, SH_C2_2 = 0.31539156525252005f, SH_C2_3 = -1.0925484305920792f, SH_C2_4 = 0.5462742152960396f;
constexpr float SH_C3_0 = -0.5900435899266435f, SH_C3_1 = 2.890611442640554f, SH_C3_2 = -0.4570457994644658f, SH_C3_3 = 0.3731763325901154f, SH_C3_4 = -0.4570457994644658f,
                SH_C3_5 = 1.445305721320277f, SH_C3_6 = -0.5900435899266435f;

constexpr uint32_t sh_coeffs(int degree) { return (uint32_t)((degree + 1) * (degree + 1)); }
constexpr uint32_t sh_pieces(int degree) { return (12u * sh_coeffs(degree) + 15u) / 16u; }       // 1, 3, 7, 12
constexpr uint32_t sh_pitch(int degree) { return sh_pieces(degree) | 1u; }                       // 1, 3, 7, 13

template <int DEGREE>
__global__ __launch_bounds__(SH_THREADS) void k_shade_sh(float4* __restrict__ rec, uint32_t n, const uint4* __restrict__ sh, uint32_t row_pieces,
                                                          float t, float camx, float camy, float camz, float4* __restrict__ plane1) {
    constexpr uint32_t K = sh_coeffs(DEGREE), Q = sh_pieces(DEGREE), P = sh_pitch(DEGREE);
    __shared__ uint4 rows[SHADE_TILE * P];
    const uint64_t rec0 = (uint64_t)blockIdx.x * SHADE_TILE;
    const uint64_t left = (uint64_t)n - rec0;                                            // (the grid has no workgroup past the end: left >= 1)
    const uint32_t slots = left < SHADE_TILE ? (uint32_t)left : SHADE_TILE, pieces = slots * Q;
    // the record side first: its two sectors travel while the table is staged (a thread past the end reads the tile's last record)
    const uint32_t r = threadIdx.x < slots ? threadIdx.x : slots - 1u;
    const uint64_t i = rec0 + r;
    const float4 pm = rec[i * 6u], sg = rec[i * 6u + 5u];
    // the table: work item j of the tile is piece j % Q of row j / Q
    const uint4* const tile = sh + rec0 * row_pieces;
    for (uint32_t j0 = threadIdx.x; j0 < pieces; j0 += 4u * SH_THREADS) {
        uint32_t row[4], piece[4];
        uint4 v[4];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            const uint32_t j = min(j0 + u * SH_THREADS, pieces - 1u);
            row[u] = j / Q;
            piece[u] = j - row[u] * Q;
        }
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) v[u] = tile[(uint64_t)row[u] * row_pieces + piece[u]];
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) if (j0 + u * SH_THREADS < pieces) rows[row[u] * P + piece[u]] = v[u];
    }
    __syncthreads();
    if (threadIdx.x >= slots) return;
    float c[4 * Q];
#pragma unroll
    for (uint32_t p = 0; p < Q; ++p) {
        // (the empty asm takes the piece whole: one 16-byte LDS read — left to itself the compiler cuts the row into 4-, 8- and 12-byte reads, which the odd pitch does not spread)
        f32x4 v = *(const f32x4*)&rows[threadIdx.x * P + p];
        asm volatile("" : "+v"(v));
        c[4 * p + 0] = v.x; c[4 * p + 1] = v.y; c[4 * p + 2] = v.z; c[4 * p + 3] = v.w;
    }
    // the direction (gs4d.h): from the camera to the time-conditioned mean the draw projects
    const float k = (1.0f / sg.w) * (t - pm.w);
    const float mx = pm.x + k * sg.x, my = pm.y + k * sg.y, mz = pm.z + k * sg.z;
    const float dx = mx - camx, dy = my - camy, dz = mz - camz;
    const float len2 = (dx * dx + dy * dy) + dz * dz;
    const bool directed = len2 > 0.0f && len2 < SH_INF;
    const float inv = 1.0f / sqrtf(len2);
    const float x = dx * inv, y = dy * inv, z = dz * inv;
    float b[16];
    b[0] = SH_C0;
    if (DEGREE >= 1) { b[1] = -SH_C1 * y; b[2] = SH_C1 * z; b[3] = -SH_C1 * x; }
    if (DEGREE >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        b[4] = SH_C2_0 * xy;
        b[5] = SH_C2_1 * yz;
        b[6] = SH_C2_2 * ((2.0f * zz - xx) - yy);
        b[7] = SH_C2_3 * xz;
        b[8] = SH_C2_4 * (xx - yy);
        if (DEGREE >= 3) {
            b[9] = (SH_C3_0 * y) * (3.0f * xx - yy);
            b[10] = (SH_C3_1 * xy) * z;
            b[11] = (SH_C3_2 * y) * ((4.0f * zz - xx) - yy);
            b[12] = (SH_C3_3 * z) * ((2.0f * zz - 3.0f * xx) - 3.0f * yy);
            b[13] = (SH_C3_4 * x) * ((4.0f * zz - xx) - yy);
            b[14] = (SH_C3_5 * z) * (xx - yy);
            b[15] = (SH_C3_6 * x) * (xx - 3.0f * yy);
        }
    }
    float out[3];
#pragma unroll
    for (uint32_t ch = 0; ch < 3u; ++ch) {
        const float dc = b[0] * c[ch];
        float acc = dc;
#pragma unroll
        for (uint32_t kk = 1; kk < K; ++kk) acc = acc + b[kk] * c[3u * kk + ch];
        const float v = (directed ? acc : dc) + 0.5f;
        out[ch] = v > 0.0f ? v : 0.0f;                                                   // (a NaN gives 0)
    }
    float* const dst = (float*)(rec + i * 6u + 1u);
    dst[0] = out[0]; dst[1] = out[1]; dst[2] = out[2];
    if (plane1) { float* const col = (float*)(plane1 + i); col[0] = out[0]; col[1] = out[1]; col[2] = out[2]; }
}

hipError_t launch_shade_sh(hipStream_t st, void* records, size_t n, const void* sh, size_t sh_stride, int degree, float t, const float cam[3], float4* plane1) {
    if (!n) return hipSuccess;
    const dim3 grid((uint32_t)((n + SHADE_TILE - 1) / SHADE_TILE)), block(SH_THREADS);
    const uint32_t row_pieces = (uint32_t)(sh_stride / 16);
#define GS4D_SHADE(D) k_shade_sh<D><<<grid, block, 0, st>>>((float4*)records, (uint32_t)n, (const uint4*)sh, row_pieces, t, cam[0], cam[1], cam[2], plane1)
    switch (degree) {
        case 0: GS4D_SHADE(0); break;
        case 1: GS4D_SHADE(1); break;
        case 2: GS4D_SHADE(2); break;
        case 3: GS4D_SHADE(3); break;
        default: return hipErrorInvalidValue;
    }
#undef GS4D_SHADE
    return hipGetLastError();
}

} // namespace gs4d
