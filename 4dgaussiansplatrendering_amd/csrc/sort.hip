// sort.hip — depth-key generation and the stable LSD radix sort (gfx950, wave64).
//
// Replaces, behind gs4d_keygen / gs4d_sort_pairs:
//   * the single-threaded CPU key loop + two uploads            4DSplatRendering/Scenes.h:28-36, 314-325
//   * radix_sort::sorter::sort and its three GLSL kernels       Dependencies/GPU_RADIX_SORT/radix_sort.hpp:258-392,
//                                                               resources/radix_sort_{count,local_offsets,reorder}.comp.glsl
// Contract kept: output == stable ascending sort by the uint32 key, payload follows (bit-exact permutation).
// Design (not a translation of the GLSL): 8-bit digits x 4 passes instead of 4-bit x 8; ONE histogram launch for all digits and
// ONE launch per pass (chained scan with decoupled look-back) instead of 2*log2(P2)+3 dispatches per pass; keys are ranked with
// wave64 ballot match + popcount (no 16 KB Blelloch tables, no per-pass re-sort of the block) and reordered in LDS so that each
// digit's run leaves the workgroup as consecutive addresses.
//
// Compiled with -ffp-contract=off: the key must be bit-identical to the CPU expression
// 1.0f / sqrtf(dx*dx + dy*dy + dz*dz) (IEEE-correct sqrt and divide are hipcc's default).
#include "gs4d_internal.h"
#include "depth_key.h"
#include <algorithm>
#include <cstdlib>
#include <cstdio>
#include <vector>

namespace gs4d {

// ------------------------------------------------------------------------------------------------
// keygen: reads 32 B/splat from the SoA planes (pos, sig[3]) instead of the 96-B record
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_keygen(const float4* __restrict__ pos, const float4* __restrict__ sig3, uint32_t n, float t,
                                                float camx, float camy, float camz, float4 vrow2 /* view row 2: V[2],V[6],V[10],V[14] */, int key_mode,
                                                float* __restrict__ keys, uint32_t* __restrict__ idx, uint32_t* __restrict__ ghist /* digit histograms of (key - bias), for the sort */, int rb /* ... in digits of rb bits */, int hist_rows, int hist_top /* SortScratch::hist_rows, hist_top */,
                                                uint32_t bias /* host-proven lower bound of every key's bit pattern */, uint32_t span /* ... and of (key - bias) from above */, uint32_t* __restrict__ err,
                                                float4 csig3, float cmut /* sig3 == nullptr (a static set: SOA_STATIC3D): sig[3] and mu_t of every record */) {
    __shared__ uint32_t h[OS_MAX_PASSES][OS_MAX_BINS];
    os_hist_clear(h, threadIdx.x);
    __syncthreads();
    for (uint32_t i0 = blockIdx.x * 256u; i0 < n; i0 += gridDim.x * 256u) {      // uniform trip count per workgroup
        const uint32_t i = i0 + threadIdx.x;
        const bool in = i < n;
        float key = 0.0f;
        if (in) {
            float4 p = pos[i];
            float4 s = csig3;
            if (sig3) s = sig3[i]; else p.w = cmut;        // uniform
            if (key_mode == GS4D_KEY_REF_INV_EUCLID) key = gs4d_key::ref_inv_euclid(p.x, p.y, p.z, p.w, s.x, s.y, s.z, t, camx, camy, camz);
            else key = gs4d_key::view_z(p.x, p.y, p.z, p.w, s.x, s.y, s.z, s.w, t, vrow2.x, vrow2.y, vrow2.z, vrow2.w);
            keys[i] = key;
            idx[i] = i;
        }
        const uint32_t kb = __float_as_uint(key);
        if (in && (kb < bias || kb - bias > span)) __hip_atomic_store(err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // the bound did not hold: reported, never silently mis-sorted
        os_hist_add(h, kb - bias, in, hist_rows, rb, hist_top);
    }
    __syncthreads();
    os_hist_flush(h, ghist, hist_rows, threadIdx.x, hist_top);
}

hipError_t launch_keygen(hipStream_t st, const float4* pos, const float4* sig3, const SoaInfo& info, size_t n, const KeySrc& ks, float* keys, uint32_t* idx, uint32_t* ghist, int rb, int hist_rows, int hist_top, uint32_t span, uint32_t* err) {
    if (n == 0) return hipSuccess;
    const float4 vr = make_float4(ks.vr0, ks.vr1, ks.vr2, ks.vr3);
    const int key_mode = ks.mode == KEYSRC_VIEWZ ? GS4D_KEY_VIEW_Z : GS4D_KEY_REF_INV_EUCLID;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 1024);     // grid-stride: bounds the histogram flush to 1024 workgroups
    k_keygen<<<dim3(blocks), dim3(256), 0, st>>>(pos, sig3, (uint32_t)n, ks.t, ks.camx, ks.camy, ks.camz, vr, key_mode, keys, idx, ghist, rb, hist_rows, hist_top, ks.bias, span, err,
                                                     make_float4(info.consts[4], info.consts[5], info.consts[6], info.consts[7]), info.consts[0]);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// radix sort: one launch per 8-bit digit, chained scan with a two-level decoupled look-back
//
//   histogram  : global digit histograms of ALL passes, [4][256].  Produced by k_os_hist (keys read once, LDS-privatised) — or,
//                for free, by the kernel that wrote the keys (k_keygen for depth keys, k_bin_emit for tile ids), in which case no
//                histogram launch happens at all.
//   k_os_pass  : a workgroup ranks the keys of its tile (wave64 ballot match), publishes its per-digit counts, looks back over its
//                predecessors to obtain its exclusive prefix, reorders the tile in LDS and writes each digit's run to its final
//                place with consecutive lanes on consecutive addresses.  Traffic per pass: keys+values read once, written once.
//   A pass whose digit is the same for every key (e.g. the sign+exponent byte of positive depth keys) is a stable identity and is
//   skipped ON THE DEVICE: every workgroup derives from the histograms which passes are live and which of three buffers (caller's,
//   scratch B, scratch C) it reads and writes, so that the last live pass lands in the caller's buffers without a copy.
// Inter-workgroup hand-off: each look-back word is ONE naturally aligned 64-bit granule {epoch:30, flag:2, value:32}, written by one
// agent-scope relaxed atomic store and polled with agent-scope relaxed atomic loads (bypass L1, write-through) — the data-tagged
// granule form of cdna_hip_programming.md Guideline 16 (R2): no separate flag, hence no ordering requirement.  The epoch (one per
// launch) makes words of earlier launches read as "not published", so the words are never zeroed.
// Look-back is two-level (tiles in groups of OS_GROUP; the last tile of a group publishes the group's total): when all tiles of a
// small sort start together, a tile needs ~3 memory round trips instead of one per ~32 predecessors.
// Tile ids are tickets (an atomic counter, one per started workgroup): a tile waits only for tiles that are already running, whatever
// the dispatch order.  Every spin is bounded as well: on time-out the kernel raises `err` and leaves, and the host reports the
// frame as failed instead of hanging the GPU or returning wrong data.
// ------------------------------------------------------------------------------------------------
// Per-tile wall-clock stamps of one pass (tools/stamps.py) exist only in tuning builds (make TUNING=1): release kernels carry no
// ablation branches.
#ifdef GS4D_TUNING
#define OS_STAMP(k) do { if (stamps && tid == 0) stamps[tile * 8 + (k)] = wall_clock64(); } while (0)
#else
#define OS_STAMP(k) do { } while (0)
#endif
constexpr uint32_t OS_GROUP = 16;         // tiles per look-back group (every look-back word in flight at once is a live register: 32 x 32 held the kernel at 177 VGPRs = one workgroup per CU)
constexpr uint32_t OS_SUPER = 16;         // groups per super-group
typedef unsigned long long u64;

struct OsBufs { uint32_t* k[3]; uint32_t* v[3]; };      // [0] caller's buffers, [1],[2] scratch

__global__ __launch_bounds__(256) void k_os_hist(const uint32_t* __restrict__ keys, uint32_t n_cap, const uint32_t* __restrict__ n_dev, int passes, int rb, int top /* >= 0: the top-digit row as well (os_hist_add) */,
                                                 uint32_t* __restrict__ ghist /* [OS_REPL][4][OS_MAX_BINS], zero on entry */) {
    __shared__ uint32_t h[OS_MAX_PASSES][OS_MAX_BINS];
    const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
    const uint32_t tid = threadIdx.x;
    os_hist_clear(h, tid);
    __syncthreads();
    const uint32_t nvec = n / 4u;
    const uint4* k4 = reinterpret_cast<const uint4*>(keys);
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t i0 = blockIdx.x * 256u + tid; i0 < nvec; i0 += 4u * stride) {
        uint4 kk[4];
        bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { const uint32_t i = i0 + u * stride; in[u] = i < nvec; kk[u] = in[u] ? k4[i] : make_uint4(0, 0, 0, 0); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            os_hist_add(h, kk[u].x, in[u], passes, rb, top); os_hist_add(h, kk[u].y, in[u], passes, rb, top);
            os_hist_add(h, kk[u].z, in[u], passes, rb, top); os_hist_add(h, kk[u].w, in[u], passes, rb, top);
        }
    }
    if (blockIdx.x == 0) { const bool in = tid < (n & 3u); os_hist_add(h, in ? keys[nvec * 4u + tid] : 0u, in, passes, rb, top); }      // tail keys
    __syncthreads();
    os_hist_flush(h, ghist, passes, tid, top);
}

// Which passes are live, and which buffers pass `p` reads and writes.  Returns false when pass p is skipped.
// A single live pass would end in a scratch buffer: one identity pass is then run as well (a stable copy), so the number of
// executed passes is 0, 2, 3 or 4 and the result always lands in buffer 0.
// `live` is a register copy of the workgroup's live mask (bit q: pass q moves keys): every thread derives the same schedule from
// the same word — nothing is amended in shared memory, so waves cannot disagree about it.
// `executed` = how many passes move keys before pass p (0: pass p is the first to read the caller's buffers), `total` = how many do at all.
__device__ __forceinline__ bool os_schedule(uint32_t live, int passes, int p, int& src, int& dst, int& executed, int& total) {
    const uint32_t all = (1u << passes) - 1u;
    live &= all;
    int k = __popc(live);
    if (k == 1) { const uint32_t deadm = all & ~live; live |= deadm & (0u - deadm); ++k; }      // revive the first dead pass (passes >= 2)
    total = k;
    const int j = __popc(live & ((1u << p) - 1u));
    executed = j;
    if (!((live >> p) & 1u)) return false;
    // buffer after i executed passes: even k: 0,1,0,1,...   odd k (>= 3): 0,1,2,0,1,0,...
    auto buf_at = [k](int i) { if (k & 1) { if (i <= 2) return i; return (i - 3) & 1; } return i & 1; };
    src = buf_at(j);
    dst = buf_at(j + 1);
    return true;
}

// ---- look-back words ----
// tile level : 32-bit {epoch:18, count:14}: the tile's count of one digit (<= TILE_KEYS < 2^14).  Published once per launch.
// group level: 64-bit {epoch:30, flag:2, value:32}: AGG = total of the group's tiles, INCL = inclusive global prefix at its end.
// Small words matter: with every tile of a 10^6-key sort in flight at once, look-back reads are (tiles^2/group) KB of uncached
// traffic per pass — as many bytes as the keys themselves if the words are wide or the tiles small.
__device__ __forceinline__ uint32_t os_tword(uint32_t epoch, uint32_t count) { return ((epoch & 0x3FFFFu) << 14) | count; }
__device__ __forceinline__ bool os_tpublished(uint32_t w, uint32_t epoch) { return (w >> 14) == (epoch & 0x3FFFFu); }

// ---- look-back reads ----
// A round of agent-scope loads costs 1.5-3 us on a busy device, so the look-back is built to need ONE: the words of the group's earlier
// tiles and the accumulators of the super-group's earlier groups are all requested before any of them is examined.
// Polling discipline when something is still missing: spin on the FIRST missing word alone (one load per thread and round, with a
// sleep), then read the rest again.  Re-reading everything every round is a polling storm — a few hundred tiles asking for tens of
// TB/s — and the stores everybody is waiting for queue up behind it.

// rows hi-k0 .. hi-(rows-1) of the tile words are outstanding and row hi-k0 is known to be missing
template <int LB, int BINS>
__device__ __forceinline__ uint32_t os_tiles_finish(const uint32_t* st, int32_t hi, int rows, int k0, uint32_t sum, uint32_t tid, uint32_t epoch, uint32_t* err) {
    uint32_t spins = 0;
    while (true) {
        while (true) {
            __builtin_amdgcn_s_sleep(8);
            const uint32_t w = __hip_atomic_load(st + (size_t)(hi - k0) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (os_tpublished(w, epoch)) { sum += w & 0x3FFFu; break; }
            if (++spins > (1u << 20)) { __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return sum; }
        }
        if (++k0 >= rows) return sum;
        uint32_t sv[LB];
#pragma unroll
        for (int k = 0; k < LB; ++k) sv[k] = (k >= k0 && k < rows) ? __hip_atomic_load(st + (size_t)(hi - k) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        bool missing = false;
#pragma unroll
        for (int k = 0; k < LB; ++k) {
            if (missing || k < k0 || k >= rows) continue;
            if (!os_tpublished(sv[k], epoch)) { k0 = k; missing = true; continue; }
            sum += sv[k] & 0x3FFFu;
        }
        if (!missing) return sum;
    }
}

// accumulator rows t+k0 .. t+rows-1 are outstanding and row t+k0 is known to be incomplete (complete = `expect` arrivals)
template <int LB, int BINS>
__device__ __forceinline__ uint32_t os_acc_finish(const uint32_t* acc, uint32_t t, int rows, int k0, uint32_t sum, uint32_t expect, uint32_t tid, uint32_t* err) {
    uint32_t spins = 0;
    while (true) {
        while (true) {
            __builtin_amdgcn_s_sleep(8);
            const uint32_t w = __hip_atomic_load(acc + (size_t)(t + k0) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((w >> 24) == expect) { sum += w & 0xFFFFFFu; break; }
            if (++spins > (1u << 20)) { __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return sum; }
        }
        if (++k0 >= rows) return sum;
        uint32_t sv[LB];
#pragma unroll
        for (int k = 0; k < LB; ++k) sv[k] = (k >= k0 && k < rows) ? __hip_atomic_load(acc + (size_t)(t + k) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        bool missing = false;
#pragma unroll
        for (int k = 0; k < LB; ++k) {
            if (missing || k < k0 || k >= rows) continue;
            if ((sv[k] >> 24) != expect) { k0 = k; missing = true; continue; }
            sum += sv[k] & 0xFFFFFFu;
        }
        if (!missing) return sum;
    }
}

// Exclusive prefix of tile `tile` for digit `tid`: earlier tiles of its group + earlier groups of its super-group + earlier super-groups.
template <int BINS>
__device__ __forceinline__ uint32_t os_lookback(const uint32_t* st, const uint32_t* acc, uint32_t acc_groups, uint32_t tile, uint32_t tid, uint32_t epoch, uint32_t* err) {
    const uint32_t grp = tile / OS_GROUP, sup = grp / OS_SUPER;
    const int rows_t = (int)(tile - grp * OS_GROUP), rows_g = (int)(grp - sup * OS_SUPER);
    const int32_t hi = (int32_t)tile - 1;
    const uint32_t g0 = sup * OS_SUPER;
    uint32_t tv[OS_GROUP], gv[OS_SUPER];
#pragma unroll
    for (int k = 0; k < (int)OS_GROUP; ++k) tv[k] = k < rows_t ? __hip_atomic_load(st + (size_t)(hi - k) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
#pragma unroll
    for (int k = 0; k < (int)OS_SUPER; ++k) gv[k] = k < rows_g ? __hip_atomic_load(acc + (size_t)(g0 + k) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    uint32_t sum_t = 0, sum_g = 0, sum_s = 0;
    int miss_t = -1, miss_g = -1;
#pragma unroll
    for (int k = 0; k < (int)OS_GROUP; ++k) {
        if (miss_t >= 0 || k >= rows_t) continue;
        if (!os_tpublished(tv[k], epoch)) { miss_t = k; continue; }
        sum_t += tv[k] & 0x3FFFu;
    }
#pragma unroll
    for (int k = 0; k < (int)OS_SUPER; ++k) {
        if (miss_g >= 0 || k >= rows_g) continue;
        if ((gv[k] >> 24) != OS_GROUP) { miss_g = k; continue; }
        sum_g += gv[k] & 0xFFFFFFu;
    }
    // earlier super-groups (sorts of more than 1024 tiles only), 16 at a time
    const uint32_t* sacc = acc + (size_t)acc_groups * (uint32_t)BINS;
    for (uint32_t t = 0; t < sup; t += 16u) {
        const int rows = (int)min(16u, sup - t);
        uint32_t sv[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) sv[k] = k < rows ? __hip_atomic_load(sacc + (size_t)(t + k) * (uint32_t)BINS + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        int miss = -1;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            if (miss >= 0 || k >= rows) continue;
            if ((sv[k] >> 24) != OS_SUPER) { miss = k; continue; }
            sum_s += sv[k] & 0xFFFFFFu;
        }
        if (miss >= 0) sum_s = os_acc_finish<16, BINS>(sacc, t, rows, miss, sum_s, OS_SUPER, tid, err);
    }
    if (miss_t >= 0) sum_t = os_tiles_finish<(int)OS_GROUP, BINS>(st, hi, rows_t, miss_t, sum_t, tid, epoch, err);
    if (miss_g >= 0) sum_g = os_acc_finish<(int)OS_SUPER, BINS>(acc, g0, rows_g, miss_g, sum_g, OS_GROUP, tid, err);
    return sum_t + sum_g + sum_s;
}

// exclusive scan of one value per digit (threads 0..BINS-1 carry a value, all THREADS threads take part in the barriers)
template <int THREADS, int BINS>
__device__ __forceinline__ uint32_t digit_excl_scan(uint32_t v, uint32_t* tmp /* __shared__[BINS / 64] */, uint32_t tid) {
    const uint32_t lane = tid & 63u, w = tid >> 6;
    const uint32_t inc = wave_incl_scan_u32(tid < (uint32_t)BINS ? v : 0u, lane);
    __syncthreads();
    if (lane == 63u && w < (uint32_t)(BINS / 64)) tmp[w] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < BINS / 64 - 1; ++k) if ((unsigned)k < w) base += tmp[k];
    return base + inc - v;
}

// ---- the tile-local part of a digit pass: rank, per-wave offsets, reorder in LDS (k_os_pass for a tile, k_os_tail for a bucket or a chunk of one) ----
// A wave looks after the keys [first, end) of the tile, item j of lane l being key first + 64 j + l (ITEMS x 64 >= end - first): wave-major, item-major,
// lane order is memory order, which is what makes the pass stable.  The digit is ((key - bias) >> shift) & mask.
// rank[j] = how many earlier keys of the wave carry the same digit; wc (the wave's row of counters, zero on entry) ends as the wave's digit counts.
template <int ITEMS, bool ATOMIC_RANK, int RB /* the ballot form's digit width: mask == (1 << RB) - 1 */>
__device__ __forceinline__ void os_rank_items(const uint32_t (&key)[ITEMS], uint32_t (&rank)[ITEMS], uint32_t first, uint32_t end, uint32_t bias, int shift, uint32_t mask, uint32_t* wcw, uint32_t lane) {
    if (ATOMIC_RANK) {
        // rank = value returned by an LDS atomic add on the wave's digit counter.  Stable only because the LDS unit serialises the
        // lanes of one instruction that hit the same counter in ascending lane order — not an architectural promise, so the
        // library verifies it on the device at context creation (k_lds_order_test) and uses the ballot form below otherwise.
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const bool valid = (first + j * 64u + lane) < end;
            const uint32_t d = ((key[j] - bias) >> shift) & mask;
            rank[j] = valid ? atomicAdd(&wcw[d], 1u) : 0u;
        }
    } else {
        const uint64_t lt = (1ull << lane) - 1ull;
        volatile uint32_t* wc = wcw;
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const bool valid = (first + j * 64u + lane) < end;
            const uint32_t d = ((key[j] - bias) >> shift) & mask;
            uint64_t m = __ballot(valid);
#pragma unroll
            for (int b = 0; b < RB; ++b) {
                const bool bit = (d >> b) & 1u;
                const uint64_t bal = __ballot(bit);
                m &= bit ? bal : ~bal;
            }
            rank[j] = 0;
            if (valid) {
                const uint32_t c = wc[d];
                rank[j] = c + (uint32_t)__popcll(m & lt);
                __builtin_amdgcn_wave_barrier();
                if ((m & lt) == 0) wc[d] = c + (uint32_t)__popcll(m);
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}
// thread d < BINS (behind a barrier after the ranking): the waves' counts of digit d become each wave's offset inside the tile's digit-d run; returns the tile's count
template <int WAVES, int BINS>
__device__ __forceinline__ uint32_t os_wave_offsets(uint32_t (*wcnt)[BINS], uint32_t tid) {
    uint32_t cnt = 0;
    if (tid < (uint32_t)BINS) {
#pragma unroll
        for (int k = 0; k < WAVES; ++k) { const uint32_t t = wcnt[k][tid]; wcnt[k][tid] = cnt; cnt += t; }
    }
    return cnt;
}
// the reorder inside LDS (behind a barrier after loff, the first local slot of every digit, was written): the tile ends in skeys / svals, digit runs in order
template <int ITEMS>
__device__ __forceinline__ void os_scatter_items(const uint32_t (&key)[ITEMS], const uint32_t (&val)[ITEMS], const uint32_t (&rank)[ITEMS], uint32_t first, uint32_t end, uint32_t bias, int shift, uint32_t mask,
                                                 const uint32_t* loff, const uint32_t* wcw, uint32_t* skeys, uint32_t* svals, uint32_t lane) {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        if ((first + j * 64u + lane) < end) {                   // stable: wave-major, item-major, lane order == memory order
            const uint32_t d = ((key[j] - bias) >> shift) & mask;
            const uint32_t l = loff[d] + wcw[d] + rank[j];
            skeys[l] = key[j];
            svals[l] = val[j];
        }
    }
}

// Persistent workgroups: the grid is what fits the device at once (or one workgroup per tile if that is fewer); a workgroup draws a
// ticket, sorts that tile, draws the next.  What does not depend on the tile (histograms -> live passes and digit bases, the
// housekeeping for the next launch) happens once per workgroup, and a finished tile's successor starts without a dispatch.
template <int THREADS, int ITEMS, bool ATOMIC_RANK, int RB>
__global__ __launch_bounds__(THREADS) void k_os_pass(OsBufs bufs, uint32_t n_cap, const uint32_t* __restrict__ n_dev, int pass, int passes,
                                                     const uint32_t* __restrict__ ghist /* [OS_REPL][4][OS_MAX_BINS] */, uint32_t* __restrict__ ghist_other /* zeroed by pass 0 */,
                                                     uint32_t* status /* [tiles][BINS] */, uint32_t* acc /* [acc_groups + supers][BINS], zero at launch */, uint32_t* acc_next /* zeroed here */, uint32_t acc_groups, uint32_t acc_words,
                                                     uint32_t epoch, uint32_t* err,
                                                     uint32_t* ticket /* zero at launch */, uint32_t* ticket_next /* zeroed here */, uint32_t bias, int identity_vals /* the payload is the identity index and has NOT been written: see radix_sort_pairs */,
                                                     int shift /* the digit is ((key - bias) >> shift) & (BINS - 1): RB * pass for an LSD pass */, int hist_row /* the row of ghist that counts this digit */,
                                                     int top /* the hybrid sort's global pass (radix_sort_pairs): always moves the keys, caller's buffers -> scratch 1, as the first executed pass */,
                                                     u64* stamps /* tuning aid, may be null */) {
    constexpr uint32_t TILE_KEYS = THREADS * ITEMS;
    constexpr int WAVES = THREADS / 64;
    constexpr uint32_t BINS = 1u << RB;                      // digits of RB bits: thread d < BINS owns digit d in everything per digit below
    static_assert(BINS <= (uint32_t)THREADS && BINS <= OS_MAX_BINS && BINS >= 64u, "one thread per digit");
    static_assert(TILE_KEYS < (1u << 14), "tile-level look-back words carry 14-bit counts");
    static_assert((uint64_t)TILE_KEYS * OS_GROUP * OS_SUPER < (1u << 24) && OS_GROUP < 256u && OS_SUPER < 256u, "accumulators are {arrivals:8, sum:24}");
    __shared__ uint32_t skeys[TILE_KEYS];
    __shared__ uint32_t svals[TILE_KEYS];
    __shared__ uint32_t wcnt[WAVES][BINS];
    __shared__ uint32_t loff[BINS];     // first local slot of digit d in the reordered tile
    __shared__ uint32_t gpos[BINS];     // global slot of that first element
    __shared__ uint32_t s_tmp[BINS / 64];
    __shared__ uint32_t s_dead;          // bit q: one digit of pass q holds every key (the pass is a stable identity)
    __shared__ uint32_t s_tile;

    const uint32_t n = n_dev ? min(*n_dev, n_cap) : n_cap;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    // Tile ids are handed out by ticket, in the order they are STARTED: a tile only ever waits for tiles that are already running.
    // (With blockIdx as the tile id, two chained-scan kernels running side by side on different streams can dead-lock each other:
    // workgroups are dispatched per XCD, so each kernel's late tiles can fill the XCD the other kernel's early tiles need.)
    // The ticket's round trip overlaps the histogram loads below, which do not depend on the tile.
    if (tid == 0) s_tile = atomicAdd(ticket, 1u);
    if (tid == 1u) s_dead = 0u;
    if (tid == 2u && blockIdx.x == 0) __hip_atomic_store(ticket_next, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // the next launch on this stream counts from zero again
    for (uint32_t q = tid; q < WAVES * BINS; q += THREADS) (&wcnt[0][0])[q] = 0u;
    uint32_t tot = 0, dead = 0;
    if (tid < BINS) {
        if (top) {                                                // (uniform) no dead-pass bookkeeping: this row is the only one counted
#pragma unroll
            for (int r = 0; r < OS_REPL; ++r) tot += ghist[(r * OS_MAX_PASSES + hist_row) * OS_MAX_BINS + tid];
        } else for (int q = 0; q < passes; ++q) {
            uint32_t g = 0;
#pragma unroll
            for (int r = 0; r < OS_REPL; ++r) g += ghist[(r * OS_MAX_PASSES + q) * OS_MAX_BINS + tid];
            if (q == hist_row) tot = g;
            if (g == n) dead |= 1u << q;                          // one digit holds every key
        }
    }
    __syncthreads();
    if (dead) atomicOr(&s_dead, dead);                            // at most one thread per dead pass
    const uint32_t ntiles = (n + TILE_KEYS - 1u) / TILE_KEYS;
    // housekeeping for the NEXT launch of this sorter: its group accumulators (every workgroup a slice), its histogram slot
    for (uint32_t q = blockIdx.x * THREADS + tid; q < acc_words; q += gridDim.x * THREADS) acc_next[q] = 0u;
    if (pass == 0 && blockIdx.x == 0) { for (uint32_t q = tid; q < OS_SLOT_WORDS; q += THREADS) ghist_other[q] = 0u; }
    __syncthreads();
    uint32_t tile = s_tile;
    if (tile >= ntiles) return;                                   // uniform
    int src = 0, dst = 1, executed = 0, total = 1;
    if (!top && !os_schedule(~s_dead, passes, pass, src, dst, executed, total)) {          // uniform: this pass is an identity
        // an identity payload nobody has written, and no pass at all will move anything (every key is the same): pass 0's launch writes it
        if (identity_vals && pass == 0 && total == 0) { for (uint32_t i = blockIdx.x * THREADS + tid; i < n; i += gridDim.x * THREADS) bufs.v[0][i] = i; }
        return;
    }
    const bool make_identity = identity_vals && executed == 0;   // uniform: the first pass that moves keys makes up the payload instead of reading it
    const uint32_t* __restrict__ keys_in = bufs.k[src]; const uint32_t* __restrict__ vals_in = bufs.v[src];
    uint32_t* __restrict__ keys_out = bufs.k[dst]; uint32_t* __restrict__ vals_out = bufs.v[dst];
    uint32_t digit_base = 0;
    bool first = true;
    const uint32_t ngroups = (ntiles + OS_GROUP - 1u) / OS_GROUP, nsuper = (ngroups + OS_SUPER - 1u) / OS_SUPER;

    while (true) {                                                // uniform: `tile` is the same in every thread
        OS_STAMP(0);
        const uint32_t tbase = tile * TILE_KEYS;
        const uint32_t wbase = tbase + w * (64u * ITEMS);
        uint32_t key[ITEMS], val[ITEMS], rank[ITEMS];
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const uint32_t i = wbase + j * 64u + lane;
            const bool valid = i < n;
            key[j] = valid ? keys_in[i] : 0xFFFFFFFFu;
            val[j] = !valid ? 0u : make_identity ? i : vals_in[i];
        }
        if (first) { digit_base = digit_excl_scan<THREADS, (int)BINS>(tot, s_tmp, tid); first = false; }      // once per workgroup, under the first tile's loads
        OS_STAMP(1);

        os_rank_items<ITEMS, ATOMIC_RANK, RB>(key, rank, wbase, n, bias, shift, BINS - 1u, wcnt[w], lane);
        __syncthreads();
        // thread d: counts per wave -> offsets inside the tile's digit-d run; tile count of digit d; publish it at once
        const uint32_t cnt = os_wave_offsets<WAVES, (int)BINS>(wcnt, tid);
        uint32_t garr = 0;
        const uint32_t grp = tile / OS_GROUP, sup = grp / OS_SUPER;
        if (tid < BINS) {
            __hip_atomic_store(status + (size_t)tile * BINS + tid, os_tword(epoch, cnt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // {arrivals:8, sum:24} accumulator of the group (only if a later tile will read it); what it held before comes back after the
            // reorder below
            // (asked for only where a super-group total will be needed: waiting for the returned value costs a memory round trip)
            if (sup + 1u < nsuper) garr = __hip_atomic_fetch_add(acc + (size_t)grp * BINS + tid, (1u << 24) | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else if (grp + 1u < ngroups) (void)__hip_atomic_fetch_add(acc + (size_t)grp * BINS + tid, (1u << 24) | cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        OS_STAMP(2);
        // local run starts, then the reorder inside LDS — none of it needs the other tiles, so it overlaps their publishing
        const uint32_t lo_ = digit_excl_scan<THREADS, (int)BINS>(cnt, s_tmp, tid);
        if (tid < BINS) loff[tid] = lo_;
        __syncthreads();
        os_scatter_items<ITEMS>(key, val, rank, wbase, n, bias, shift, BINS - 1u, loff, wcnt[w], skeys, svals, lane);
        OS_STAMP(3);
        if (tid < BINS) {
            // the tile that completes its group (per digit: whichever arrived sixteenth) hands the group's total to the super-group: a
            // super-group's accumulator takes OS_SUPER additions per digit, not one from every tile under it
            if (sup + 1u < nsuper && (garr >> 24) == OS_GROUP - 1u)
                (void)__hip_atomic_fetch_add(acc + (size_t)(acc_groups + sup) * BINS + tid, (1u << 24) | ((garr & 0xFFFFFFu) + cnt), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // look back, one memory round trip: the tiles of this group before this one (their words), the groups of this super-group
            // before this group and the super-groups before this one (their accumulators, complete when every member has arrived)
            const uint32_t prefix = os_lookback<(int)BINS>(status, acc, acc_groups, tile, tid, epoch, err);
            gpos[tid] = digit_base + prefix;
        }
        __syncthreads();
        OS_STAMP(4);
        const uint32_t tcount = min(TILE_KEYS, n - tbase);
#pragma unroll
        for (int j = 0; j < ITEMS; ++j) {
            const uint32_t l = j * THREADS + tid;
            if (l < tcount) {
                const uint32_t k = skeys[l];
                const uint32_t d = ((k - bias) >> shift) & (BINS - 1u);
                const uint32_t o = gpos[d] + (l - loff[d]);
                // Small sorts (one round of tiles): streaming stores, the runs go to memory as they are written instead of sitting dirty in
                // this XCD's L2 until the end-of-kernel write-back.  Large sorts (the 8192-key shape, several rounds of tiles per workgroup):
                // ordinary stores, so that the L2 merges the partial lines at the ends of neighbouring runs before they reach HBM — measured
                // at 10^7 keys: 75.7 -> 57.7 us per pass; at 10^6 keys the streaming form is the faster one (14.1 against 15.8).
                // `o` is built from the global digit histograms, which an EARLIER kernel accumulated (k_keygen, the projection, k_os_hist), and
                // from this launch's own counts: if the keys changed in between — a caller refilling the buffer through a device pointer
                // without gs4d_buffer_invalidate — the two no longer describe the same array and `o` can point anywhere.  One compare keeps
                // the store inside the buffer and turns the contract violation into the error word (the frame is reported as failed).
                if (o >= n) { __hip_atomic_store(err, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); continue; }
                if (ITEMS >= 12) { keys_out[o] = k; vals_out[o] = svals[l]; }
                else { __builtin_nontemporal_store(k, keys_out + o); __builtin_nontemporal_store(svals[l], vals_out + o); }
            }
        }
        OS_STAMP(5);
        // The next ticket is drawn only now, behind the write-out: tiles with later tickets wait for the tile it names to publish, so a
        // ticket must not be held while its holder is still busy with something else (drawn before the write-out, 8 us at 10^7 keys, every
        // successor's look-back waited that long).  The other workgroup of the CU covers the round trip.
        if (gridDim.x >= ntiles) return;                          // uniform: every tile has a workgroup of its own, nothing is left to draw
        uint32_t next = 0;
        if (tid == 0) next = atomicAdd(ticket, 1u);
        __syncthreads();                                          // everybody is done with the tile's LDS
        if (tid == 0) s_tile = next;
        for (uint32_t q = tid; q < WAVES * BINS; q += THREADS) (&wcnt[0][0])[q] = 0u;
        __syncthreads();
        tile = s_tile;
        if (tile >= ntiles) return;                               // uniform; every workgroup ends on a ticket past the last tile
    }
}

// Does an LDS atomic add executed by a whole wave return, to the lanes that hit the same address, their rank in ascending lane order?
__global__ __launch_bounds__(256) void k_lds_order_test(uint32_t* __restrict__ bad) {
    __shared__ uint32_t cnt[4][256];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    uint32_t errors = 0;
    for (uint32_t round = 0; round < 96u; ++round) {
#pragma unroll
        for (int k = 0; k < 4; ++k) cnt[k][tid] = 0u;
        __syncthreads();
        const uint32_t bins = round % 6u == 0u ? 1u : round % 6u == 1u ? 2u : round % 6u == 2u ? 3u : round % 6u == 3u ? 7u : round % 6u == 4u ? 64u : 256u;
        uint32_t x = (blockIdx.x * 256u + tid) * 2654435761u + round * 40503u; x ^= x >> 15; x *= 2246822519u; x ^= x >> 13;
        const uint32_t d = x % bins;
        const bool active = ((x >> 20) & 7u) != 0u;              // some lanes sit out, as at the end of an array
        uint64_t m = __ballot(active);
#pragma unroll
        for (int b = 0; b < 8; ++b) { const bool bit = (d >> b) & 1u; const uint64_t bal = __ballot(bit); m &= bit ? bal : ~bal; }
        if (active) {
            const uint32_t got = atomicAdd(&cnt[w][d], 1u);
            const uint32_t want = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (got != want) ++errors;
            const uint32_t got2 = atomicAdd(&cnt[w][d], 1u);     // a second instruction continues after all lanes of the first
            if (got2 != (uint32_t)__popcll(m) + want) ++errors;
        }
        __syncthreads();
    }
    if (errors) atomicAdd(bad, errors);
}

// The test runs on every stream given, at the same time (the frame lanes' streams sit on hardware queues of their own): the workgroups of the
// launches share the CUs, so each wave is ranked beside waves of another kernel instance — the situation the product's kernels are in.
hipError_t lds_atomic_order_selftest(const hipStream_t* streams, int nstreams, bool* ordered) {
    *ordered = false;
    if (nstreams < 1) return hipErrorInvalidValue;
    if (nstreams > 8) nstreams = 8;
    uint32_t* d = nullptr; uint32_t h[8] = { 1, 1, 1, 1, 1, 1, 1, 1 };
    hipError_t e = hipMalloc(&d, 4 * (size_t)nstreams);
    if (e != hipSuccess) return e;
    for (int i = 0; i < nstreams && e == hipSuccess; ++i) e = hipMemsetAsync(d + i, 0, 4, streams[i]);
    for (int i = 0; i < nstreams && e == hipSuccess; ++i) { k_lds_order_test<<<dim3(512), dim3(256), 0, streams[i]>>>(d + i); e = hipGetLastError(); }
    for (int i = 0; i < nstreams && e == hipSuccess; ++i) e = hipMemcpyAsync(&h[i], d + i, 4, hipMemcpyDeviceToHost, streams[i]);
    for (int i = 0; i < nstreams; ++i) { const hipError_t e2 = hipStreamSynchronize(streams[i]); if (e == hipSuccess) e = e2; }
    (void)hipFree(d);
    bool ok = e == hipSuccess;
    for (int i = 0; i < nstreams; ++i) ok = ok && h[i] == 0;
    *ordered = ok;
    return e;
}

// ------------------------------------------------------------------------------------------------
// The MSD/LSD hybrid for depth keys whose host-proven span is 19..27 bits (sort_plan_hist): two launches instead of three or four chained passes.
//   launch A : k_os_pass<512, 12, true, 9> with `top` set: ONE global pass on the 9-bit top digit (key - bias) >> (key_bits - 9), caller's buffers
//              (identity payload made up) -> scratch 1.  The array is then cut into at most 512 buckets, each still in the caller's order.
//   launch B : k_os_tail, one workgroup per top digit.  The bucket's range comes from an exclusive scan of the top-digit histogram (no look-back, no
//              global atomic); the bucket is loaded into LDS, its remaining key_bits - 9 bits are sorted by two stable local passes (the tile-local
//              ranking of k_os_pass) and it goes back, coalesced, to the same range of the caller's buffers.
// No workgroup of launch B waits for another one: no spin, no ticket, no persistent grid.
// A bucket above `cap` keys (the LDS tile, or GS4D_SORT_TAILCAP) is sorted by the same workgroup with two LSD passes through global memory, in chunks
// of OT_TILE keys taken in order with running digit offsets: scratch 1 -> scratch 2 -> caller's buffers, __syncthreads only.  Slow (one workgroup,
// linear in the bucket) but exact.  The first workgroup reports the largest bucket and the number of such buckets to the host (os_top_report): a
// crowded key distribution makes the host plan the LSD passes for the next sorts instead (sort_plan_hist).
// ------------------------------------------------------------------------------------------------
constexpr int OT_THREADS = 512, OT_ITEMS = 16, OT_WAVES = OT_THREADS / 64, OT_BINS = 512;
constexpr uint32_t OT_TILE = OT_THREADS * OT_ITEMS;      // 8192 keys: the largest bucket sorted inside LDS, and the slow path's chunk
static_assert(OT_BINS == (int)OS_MAX_BINS && OT_BINS <= OT_THREADS, "one thread per top digit and per local digit");
// LB = bins of the local passes: 256 while both local digits are <= 8 bits (spans of <= 25 bits: the counters, offsets and running positions then leave the
// workgroup under 80 KB of LDS, two workgroups per CU), 512 for 26- and 27-bit spans
static_assert(OS_TOP_ROW >= 3, "SortScratch::hist_rows: a span of <= 27 bits has three LSD rows below the top-digit row");

// thread d carries g = the count of top digit d; the workgroup's thread 0 writes the report (pinned host memory)
__device__ __forceinline__ void os_top_report(uint32_t g, uint32_t cap, uint32_t* red /* __shared__[2 * OT_WAVES] */, uint32_t* fb, uint32_t tid) {
    uint32_t mx = g, slow = g > cap ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { mx = max(mx, (uint32_t)__shfl_xor(mx, off, 64)); slow += (uint32_t)__shfl_xor(slow, off, 64); }
    if ((tid & 63u) == 0u) { red[tid >> 6] = mx; red[OT_WAVES + (tid >> 6)] = slow; }
    __syncthreads();
    if (tid == 0u) {
#pragma unroll
        for (int k = 1; k < OT_WAVES; ++k) { mx = max(mx, red[k]); slow += red[OT_WAVES + k]; }
        __hip_atomic_store(fb + 0, mx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(fb + 1, slow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(fb + 2, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__device__ __forceinline__ uint32_t os_top_count(const uint32_t* __restrict__ ghist, uint32_t tid) {
    uint32_t g = 0;
#pragma unroll
    for (int r = 0; r < OS_REPL; ++r) g += ghist[(r * OS_MAX_PASSES + OS_TOP_ROW) * OS_MAX_BINS + tid];
    return g;
}
// the report alone, behind the LSD passes of a sort that is eligible for the hybrid but crowded: how the plan finds its way back
__global__ __launch_bounds__(OT_THREADS) void k_os_top_stats(const uint32_t* __restrict__ ghist, uint32_t cap, uint32_t* fb) {
    __shared__ uint32_t red[2 * OT_WAVES];
    os_top_report(os_top_count(ghist, threadIdx.x), cap, red, fb, threadIdx.x);
}

// One stable pass on the digit ((key - bias) >> shift) & mask over the `count` (<= OT_TILE) keys the workgroup holds in registers (wave w: keys
// [first, end) of them, os_rank_items' layout): they end in skeys / svals, loff[d] is the first slot of digit d.  Returns the count of digit `tid`.
template <int LB>
__device__ __forceinline__ uint32_t ot_local_pass(const uint32_t (&key)[OT_ITEMS], const uint32_t (&val)[OT_ITEMS], uint32_t first, uint32_t end, uint32_t bias, int shift, uint32_t mask,
                                                  uint32_t (*wcnt)[LB], uint32_t* loff, uint32_t* s_tmp, uint32_t* skeys, uint32_t* svals, uint32_t tid) {
    const uint32_t lane = tid & 63u, w = tid >> 6;
    uint32_t rank[OT_ITEMS];
    for (uint32_t q = tid; q < (uint32_t)(OT_WAVES * LB); q += OT_THREADS) (&wcnt[0][0])[q] = 0u;
    __syncthreads();                                              // (also: everybody has read what it wanted of skeys / svals / loff)
    os_rank_items<OT_ITEMS, true, 9>(key, rank, first, end, bias, shift, mask, wcnt[w], lane);
    __syncthreads();
    const uint32_t cnt = os_wave_offsets<OT_WAVES, LB>(wcnt, tid);
    const uint32_t lo = digit_excl_scan<OT_THREADS, LB>(cnt, s_tmp, tid);
    if (tid < (uint32_t)LB) loff[tid] = lo;
    __syncthreads();
    os_scatter_items<OT_ITEMS>(key, val, rank, first, end, bias, shift, mask, loff, wcnt[w], skeys, svals, lane);
    __syncthreads();
    return cnt;
}
// the keys [first, end) of `count` (<= OT_TILE) that wave w looks after: equal shares, whole rows of 64 lanes
__device__ __forceinline__ void ot_wave_range(uint32_t count, uint32_t w, uint32_t& first, uint32_t& end) {
    const uint32_t share = (((count + OT_WAVES - 1u) / OT_WAVES) + 63u) & ~63u;      // <= 64 * OT_ITEMS
    first = w * share;
    end = min(count, first + share);                              // (a wave past the end: end <= first, nothing valid)
}

// The segment-fed source (SEG): bucket d is not a range of scratch 1 but one run per segment of the staged projection (k_project_count<SRC, Stage, SegmentFed>,
// preprocess.hip), each inside that segment's block of seg_pairs.  s_word[r] = count | offset << 12 of segment r's run, s_first[r] = the runs before it: the
// runs go to dk / dv[s_first[r] ...] in segment order — segments in record order, a run stable in record order: the bucket in the caller's order, as launch A
// leaves it.  Eight lanes share a run (about four pairs at 10^6 keys: 489 segments x 512 digits), eight runs per lane are in flight at once, eight pairs of each a round
// (correct at any length up to the block's 2048).
struct OsSegSrc { const uint2* pairs; const uint32_t* runs; uint32_t rows; uint32_t* ghist_other; };
__device__ __forceinline__ void ot_gather_runs(const uint2* __restrict__ pairs, uint32_t rows, const uint32_t* s_word, const uint32_t* s_first, uint32_t* dk, uint32_t* dv, uint32_t tid) {
    constexpr int U = 8;                                          // runs a lane works on at once: 512 segments per step of the outer loop
    const uint32_t sub = tid & 7u;
    for (uint32_t r0 = tid >> 3; r0 < rows; r0 += (OT_THREADS / 8) * U) {
        uint2 v[U]; uint32_t cnt[U], dst[U], src[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t r = r0 + (uint32_t)u * (OT_THREADS / 8);
            const bool in = r < rows;
            const uint32_t wd = in ? s_word[r] : 0u;
            cnt[u] = wd & 0xFFFu; dst[u] = in ? s_first[r] : 0u; src[u] = r * SEGFEED_BLOCK + (wd >> 12);
            // (a word from a table the producer did not write for these keys could point anywhere: the run stays inside its block whatever it says)
            if ((wd >> 12) + cnt[u] > SEGFEED_BLOCK) cnt[u] = 0u;
        }
        uint32_t longest = 0u;
#pragma unroll
        for (int u = 0; u < U; ++u) longest = max(longest, cnt[u]);
        // Eight pairs of every run a round, until the longest of the lane's runs is through: all loads of a round are asked for before the first is stored, so
        // a round is one memory round trip — the densest bucket (runs of 14 pairs on average at 10^6 keys) decides how long the launch takes
        for (uint32_t k = sub; k - sub < longest; k += 8u) {
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = k < cnt[u] ? pairs[src[u] + k] : make_uint2(0u, 0u);
#pragma unroll
            for (int u = 0; u < U; ++u) if (k < cnt[u]) { dk[dst[u] + k] = v[u].x; dv[dst[u] + k] = v[u].y; }
        }
    }
}

template <int LB, bool SEG>
__global__ __launch_bounds__(OT_THREADS) void k_os_tail(OsBufs bufs, uint32_t n, const uint32_t* __restrict__ ghist /* the slot launch A read */, uint32_t bias,
                                                        int rem /* key bits below the top digit: 10..18 */, uint32_t cap /* <= OT_TILE */, uint32_t* fb, uint32_t* err, OsSegSrc seg) {
    __shared__ uint32_t skeys[OT_TILE];
    __shared__ uint32_t svals[OT_TILE];
    __shared__ uint32_t wcnt[OT_WAVES][LB];
    __shared__ uint32_t loff[LB];
    __shared__ uint32_t gpos[LB];
    __shared__ uint32_t s_run[2][LB];           // slow path: where the next key of each digit goes, per pass
    __shared__ uint32_t s_tmp[OT_BINS / 64];
    __shared__ uint32_t s_red[2 * OT_WAVES];
    __shared__ uint32_t s_range[3];
    static_assert(!SEG || OT_WAVES * LB >= 2 * (int)SEGFEED_MAX_ROWS, "the run words and their prefix borrow wcnt before the first local pass clears it");
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    // segment-fed: this digit's row of the run table, two segments per thread — asked for together with the histogram (neither depends on the other)
    uint32_t wa = 0u, wb = 0u;
    if (SEG) {
        const uint32_t* __restrict__ row = seg.runs + (size_t)blockIdx.x * seg.rows;
        if (2u * tid < seg.rows) wa = row[2u * tid];
        if (2u * tid + 1u < seg.rows) wb = row[2u * tid + 1u];
    }
    {
        const uint32_t g = os_top_count(ghist, tid);
        const uint32_t excl = digit_excl_scan<OT_THREADS, OT_BINS>(g, s_tmp, tid);
        if (tid == blockIdx.x) { s_range[0] = excl; s_range[1] = g; }
        if (blockIdx.x == 0) os_top_report(g, cap, s_red, fb, tid);      // uniform
        // no k_os_pass runs in a segment-fed sort: the housekeeping its first launch does for the next sort — a clean histogram slot — is done here, every workgroup a slice
        if (SEG) { constexpr uint32_t SLICE = (uint32_t)(OS_SLOT_WORDS / OT_BINS); static_assert(SLICE * OT_BINS == OS_SLOT_WORDS && SLICE <= OT_THREADS, "a slice per workgroup"); if (tid < SLICE) seg.ghist_other[blockIdx.x * SLICE + tid] = 0u; }
        __syncthreads();
    }
    const uint32_t start = s_range[0], count = s_range[1];
    if (count == 0u) return;                                      // uniform: an empty bucket
    // the histogram and the keys no longer describe the same array (see k_os_pass's write-out): nothing outside [0, n) is touched
    if (start > n || count > n - start) { if (tid == 0u) __hip_atomic_store(err, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return; }
    if (SEG) {
        // the runs must add up to the histogram's count (else the table and the histogram are not of the same keys)
        uint32_t* const s_word = &wcnt[0][0]; uint32_t* const s_first = s_word + SEGFEED_MAX_ROWS;
        const uint32_t r = 2u * tid;
        const uint32_t ca = wa & 0xFFFu, cb = wb & 0xFFFu;
        const uint32_t before = digit_excl_scan<OT_THREADS, OT_BINS>(ca + cb, s_tmp, tid);
        s_word[r] = wa; s_word[r + 1u] = wb; s_first[r] = before; s_first[r + 1u] = before + ca;
        if (tid == OT_THREADS - 1u) s_range[2] = before + ca + cb;
        __syncthreads();
        if (s_range[2] != count) { if (tid == 0u) __hip_atomic_store(err, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); return; }      // uniform
        if (count <= cap) ot_gather_runs(seg.pairs, seg.rows, s_word, s_first, skeys, svals, tid);      // free: a local pass writes them only after ranking from registers
        else ot_gather_runs(seg.pairs, seg.rows, s_word, s_first, bufs.k[1] + start, bufs.v[1] + start, tid);      // the slow path's source: this bucket's own range of scratch 1
        __threadfence_block();
        __syncthreads();
    }
    const int w0 = (rem + 1) >> 1, w1 = rem >> 1;                 // the two local digits: bits [0, w0) and [w0, rem), each <= 9 bits
    const uint32_t m0 = (1u << w0) - 1u, m1 = (1u << w1) - 1u;
    uint32_t key[OT_ITEMS], val[OT_ITEMS];
    if (count <= cap) {
        // ---- the bucket fits: load, two local passes, write back ----
        const uint32_t* k1 = SEG ? skeys : bufs.k[1] + start; const uint32_t* v1 = SEG ? svals : bufs.v[1] + start;
        uint32_t first, end;
        ot_wave_range(count, w, first, end);
#pragma unroll
        for (int j = 0; j < OT_ITEMS; ++j) {
            const uint32_t i = first + j * 64u + lane;
            const bool valid = i < end;
            key[j] = valid ? k1[i] : 0xFFFFFFFFu;
            val[j] = valid ? v1[i] : 0u;
        }
        (void)ot_local_pass<LB>(key, val, first, end, bias, 0, m0, wcnt, loff, s_tmp, skeys, svals, tid);
#pragma unroll
        for (int j = 0; j < OT_ITEMS; ++j) {
            const uint32_t i = first + j * 64u + lane;
            if (i < end) { key[j] = skeys[i]; val[j] = svals[i]; }
        }
        (void)ot_local_pass<LB>(key, val, first, end, bias, w0, m1, wcnt, loff, s_tmp, skeys, svals, tid);      // (its first barrier stands between the reads above and its writes)
        uint32_t* k0 = bufs.k[0] + start; uint32_t* v0 = bufs.v[0] + start;
        for (uint32_t l = tid; l < count; l += OT_THREADS) { k0[l] = skeys[l]; v0[l] = svals[l]; }
        return;
    }
    // ---- the bucket does not fit: two LSD passes through global memory, chunk by chunk ----
    if (tid < (uint32_t)LB) { s_run[0][tid] = 0u; s_run[1][tid] = 0u; }
    __syncthreads();
    {
        const uint32_t* k1 = bufs.k[1] + start;
        for (uint32_t i = tid; i < count; i += OT_THREADS) {
            const uint32_t k = k1[i] - bias;
            atomicAdd(&s_run[0][k & m0], 1u);
            atomicAdd(&s_run[1][(k >> w0) & m1], 1u);
        }
    }
    __syncthreads();
    {
        const bool mine = tid < (uint32_t)LB;
        const uint32_t a = mine ? s_run[0][tid] : 0u, b = mine ? s_run[1][tid] : 0u;
        const uint32_t ea = digit_excl_scan<OT_THREADS, LB>(a, s_tmp, tid);
        const uint32_t eb = digit_excl_scan<OT_THREADS, LB>(b, s_tmp, tid);
        if (mine) { s_run[0][tid] = ea; s_run[1][tid] = eb; }      // (every thread its own words)
    }
    __syncthreads();
    for (int p = 0; p < 2; ++p) {
        const uint32_t* kin = bufs.k[p + 1] + start; const uint32_t* vin = bufs.v[p + 1] + start;
        uint32_t* kout = bufs.k[p == 0 ? 2 : 0] + start; uint32_t* vout = bufs.v[p == 0 ? 2 : 0] + start;
        const int shift = p == 0 ? 0 : w0;
        const uint32_t mask = p == 0 ? m0 : m1;
        for (uint32_t c0 = 0; c0 < count; c0 += OT_TILE) {       // uniform
            const uint32_t cc = min(OT_TILE, count - c0);
            uint32_t first, end;
            ot_wave_range(cc, w, first, end);
#pragma unroll
            for (int j = 0; j < OT_ITEMS; ++j) {
                const uint32_t i = first + j * 64u + lane;
                const bool valid = i < end;
                key[j] = valid ? kin[c0 + i] : 0xFFFFFFFFu;
                val[j] = valid ? vin[c0 + i] : 0u;
            }
            const uint32_t cnt = ot_local_pass<LB>(key, val, first, end, bias, shift, mask, wcnt, loff, s_tmp, skeys, svals, tid);
            if (tid < (uint32_t)LB) { gpos[tid] = s_run[p][tid]; s_run[p][tid] += cnt; }      // the chunks come in order: digit d's keys of this chunk follow those of the chunks before
            __syncthreads();
            for (uint32_t l = tid; l < cc; l += OT_THREADS) {
                const uint32_t k = skeys[l];
                const uint32_t d = ((k - bias) >> shift) & mask;
                const uint32_t o = gpos[d] + (l - loff[d]);
                if (o >= count) { __hip_atomic_store(err, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); continue; }      // the keys changed under the sort
                kout[o] = k; vout[o] = svals[l];
            }
            __syncthreads();                                      // the chunk's LDS is free again
        }
        __syncthreads();                                          // the pass's stores are visible to the whole workgroup before the next pass loads them
    }
}

hipError_t sort_scratch_reserve(hipStream_t st, SortScratch& s, size_t n) {
    hipError_t e;
    if (s.cap < n) {
        e = grow_device_array(st, s.keys2, s.cap, n, 16);        // scratch B and C, keys and values
        s.vals2 = s.keys2 ? s.keys2 + 2 * s.cap : nullptr;
        if (e != hipSuccess) return e;
    }
    // the segment blocks and the run table of a segment-fed sort (8 bytes a key + 2 KB a segment), for sorts a staged projection can produce: at most
    // SEGFEED_MAX_ROWS segments of SEGFEED_BLOCK records (tile_lists_plan).  Both sized for n alone: sort_plan_hist checks the producer's segments against them.
    if (s.segfeed && n <= (size_t)SEGFEED_MAX_ROWS * SEGFEED_BLOCK) {
        const size_t rows = (n + SEGFEED_BLOCK - 1) / SEGFEED_BLOCK;
        if ((e = grow_device_array(st, s.seg_pairs, s.seg_cap, rows * SEGFEED_BLOCK)) != hipSuccess) return e;
        if ((e = grow_device_array(st, s.seg_runs, s.runs_cap, rows * OS_MAX_BINS)) != hipSuccess) return e;
    }
    // control block: two [OS_REPL][4][OS_MAX_BINS] histogram slots (alternating), then the look-back words [tiles + groups][bins], sized for the widest digit
    const size_t tiles = (s.cap + 1023) / 1024;      // smallest tile = 1024 keys; sized for the largest sort seen (the layout depends on it)
    const size_t groups = tiles / OS_GROUP + 2, supers = groups / OS_SUPER + 2;
    const size_t words = 2 * OS_SLOT_WORDS + (tiles + 2 + 2 * 2 * (groups + supers)) * OS_MAX_BINS;       // tile words, two accumulator sets
    if (s.hist_cap < words) {      // (not grow_device_array: the new block is filled from the old one before that is let go)
        uint32_t* nh = nullptr;
        if ((e = hipMalloc(&nh, words * 4)) != hipSuccess) return e;
        if ((e = hipMemsetAsync(nh, 0, words * 4, st)) != hipSuccess) return e;
        if (s.hist) {
            // keep a histogram that a producer kernel has already accumulated into the current slot
            if ((e = hipMemcpyAsync(nh, s.hist, 2 * OS_SLOT_WORDS * 4, hipMemcpyDeviceToDevice, st)) != hipSuccess) return e;
            (void)hipStreamSynchronize(st); (void)hipFree(s.hist);
        }
        s.hist = nh; s.hist_cap = words;
    }
    if (!s.totals) {
        // test hook: start the epoch counter close to its 18-bit wrap so that a short test crosses it
        if (const char* e0 = getenv("GS4D_TEST_EPOCH0")) s.epoch = (uint32_t)strtoul(e0, nullptr, 0);
    }
    if (!s.totals) { if ((e = hipMalloc(&s.totals, 256 * 4)) != hipSuccess) return e; if ((e = hipMemsetAsync(s.totals, 0, 1024, st)) != hipSuccess) return e; }
    if (!s.fb) {      // the top-digit report words: pinned + mapped, like the draws' verdict words
        if ((e = hipHostMalloc((void**)&s.fb, 4 * 4, hipHostMallocMapped)) != hipSuccess) { s.fb = nullptr; return e; }
        s.fb[0] = s.fb[1] = s.fb[2] = s.fb[3] = 0u;
        if ((e = hipHostGetDevicePointer((void**)&s.fb_dev, s.fb, 0)) != hipSuccess) { (void)hipHostFree(s.fb); s.fb = s.fb_dev = nullptr; return e; }
    }
    return hipSuccess;
}

void sort_scratch_free(SortScratch& s) {
    if (s.keys2) (void)hipFree(s.keys2);
    if (s.hist) (void)hipFree(s.hist);
    if (s.seg_pairs) (void)hipFree(s.seg_pairs);
    if (s.seg_runs) (void)hipFree(s.seg_runs);
    if (s.totals) (void)hipFree(s.totals);
    if (s.fb) (void)hipHostFree(s.fb);
    s = SortScratch();
}

uint32_t* sort_hist_slot(hipStream_t st, SortScratch& s, size_t n_hint, hipError_t* e_out) {
    // The slot a producer kernel (k_keygen, k_bin_emit) accumulates the digit histograms of the NEXT sort into.  It is zero unless an
    // earlier producer's histogram was never consumed by a sort; then it is cleared first.
    hipError_t e = sort_scratch_reserve(st, s, n_hint);
    if (e == hipSuccess && s.hist_pending) e = hipMemsetAsync(s.hist + (s.flip ? OS_SLOT_WORDS : 0), 0, OS_SLOT_WORDS * 4, st);
    if (e_out) *e_out = e;
    if (e != hipSuccess) return nullptr;
    s.hist_pending = true;
    return s.hist + (s.flip ? OS_SLOT_WORDS : 0);
}

// what a sort executes: LSD digit rows counted (OS_MAX_PASSES: the plain plan), the top digit's shift (-1: not counted), and whether it is the hybrid
// segfeed: the hybrid's buckets come from the producer's segment blocks (seg_rows segments), launch A does not run
struct OsPlan { int rows = OS_MAX_PASSES; int top = -1; bool hybrid = false; bool segfeed = false; uint32_t seg_rows = 0; };
static uint32_t os_tail_cap(const SortScratch& s) { return std::min<uint32_t>(std::max<uint32_t>(s.tail_cap, 1u), OT_TILE); }
static OsPlan os_plan(const SortScratch& s, size_t n, int key_bits) {
    OsPlan p;
    const bool eligible = s.hybrid_knob != 0 && key_bits >= 19 && key_bits <= 27 && s.atomic_rank && s.rank_knob != 1 && !s.rb_knob && !s.shape_knob && s.fb &&
                          n >= 2 && (s.hybrid_knob == 1 || n >= OS_HYBRID_MIN_N);
    if (!eligible) return p;
    p.top = key_bits - 9;
    // the latest report the host has seen (no wait: a wrong guess costs slow sorts, never a wrong result)
    const bool crowded = __atomic_load_n(&s.fb[2], __ATOMIC_RELAXED) != 0u && __atomic_load_n(&s.fb[0], __ATOMIC_RELAXED) > os_tail_cap(s);
    if (crowded) p.rows = sort_plan_passes(key_bits, sort_plan_rb(s, n, key_bits));      // three LSD rows, the top digit beside them
    else { p.rows = 0; p.hybrid = true; }
    return p;
}

template <int THREADS, int ITEMS, bool ATOMIC_RANK, int RB>
static hipError_t onesweep(hipStream_t st, SortScratch& s, uint32_t* keys, uint32_t* vals, size_t n, const uint32_t* n_dev, int passes, bool have_hist, bool identity_vals, const OsPlan& plan) {
    const uint32_t tile_keys = THREADS * ITEMS;
    const uint32_t tiles = (uint32_t)((n + tile_keys - 1) / tile_keys);
    // persistent workgroups: as many as the device holds at once (asked of the runtime once per scratch and kernel instance: the scratch's context has
    // made its device current)
    uint32_t resident = 0;
    {
        const void* const fn = reinterpret_cast<const void*>(&k_os_pass<THREADS, ITEMS, ATOMIC_RANK, RB>);
        SortScratch::Resident* slot = nullptr;
        for (auto& r : s.resident) { if (r.fn == fn) { resident = r.groups; break; } if (!r.fn && !slot) slot = &r; }
        if (!resident) {
            int per_cu = 0, dev = 0, cus = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_os_pass<THREADS, ITEMS, ATOMIC_RANK, RB>, THREADS, 0) != hipSuccess || per_cu < 1) per_cu = 1;
            if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
            resident = (uint32_t)per_cu * (uint32_t)cus;
            if (slot) { slot->fn = fn; slot->groups = resident; }
        }
    }
    const uint32_t grid = std::min(tiles, resident);
    uint32_t* ghist = s.hist + (s.flip ? OS_SLOT_WORDS : 0);
    uint32_t* ghist_other = s.hist + (s.flip ? 0 : OS_SLOT_WORDS);
    hipError_t e;
    const uint32_t bias = have_hist ? s.hist_bias : 0u;
    s.hist_bias = 0;
    if (!have_hist) {
        if (s.hist_pending) { if ((e = hipMemsetAsync(ghist, 0, OS_SLOT_WORDS * 4, st)) != hipSuccess) return e; }   // someone else's histogram sits in the slot
        const uint32_t hist_blocks = (uint32_t)std::min<size_t>((n / 16 + 255) / 256 + 1, 256);          // few workgroups: each flushes 256 global atomics per pass
        k_os_hist<<<dim3(hist_blocks), dim3(256), 0, st>>>(keys, (uint32_t)n, n_dev, plan.rows < OS_MAX_PASSES ? plan.rows : passes, RB, plan.top, ghist);
        ++s.stat_launches;
    }
    s.hist_pending = false;
    s.flip ^= 1;
#ifdef GS4D_TUNING
    static const char* stampf = getenv("GS4D_SORT_STAMP_FILE");
    static const int stamp_pass = getenv("GS4D_SORT_STAMP_PASS") ? atoi(getenv("GS4D_SORT_STAMP_PASS")) : 0;
#else
    const char* stampf = nullptr; const int stamp_pass = 0;
#endif
    u64* stamps = nullptr;
    if (stampf && hipMalloc(&stamps, (size_t)tiles * 64) != hipSuccess) stamps = nullptr;
    uint32_t* status = s.hist + 2 * OS_SLOT_WORDS;
    // accumulator sets sit behind the tile words of the LARGEST sort this scratch was sized for (so they never move between launches)
    const size_t cap_tiles = (s.cap + 1023) / 1024, cap_groups = cap_tiles / OS_GROUP + 2, cap_supers = cap_groups / OS_SUPER + 2;
    const size_t acc_words = (cap_groups + cap_supers) * OS_MAX_BINS;
    uint32_t* acc_base = status + (cap_tiles + 2) * OS_MAX_BINS;
    OsBufs b;
    b.k[0] = keys; b.v[0] = vals;
    b.k[1] = s.keys2; b.v[1] = s.vals2;
    b.k[2] = s.keys2 + s.cap; b.v[2] = s.vals2 + s.cap;
    // the hybrid: ONE launch of the pass kernel, on the top digit (the row the producer counted), then the tail; a fallback sort: the report behind its passes
    const int launches = plan.segfeed ? 0 : plan.hybrid ? 1 : passes;      // (segment-fed: no pass launch — the epoch and the accumulator sets stay where they are)
    for (int p = 0; p < launches; ++p) {
        ++s.epoch;
        if ((s.epoch & 0x3FFFFu) == 0u) {    // the 18-bit tile-level epoch wraps: forget every old word
            if ((e = hipMemsetAsync(status, 0, (s.hist_cap - 2 * OS_SLOT_WORDS) * 4, st)) != hipSuccess) return e;
            ++s.epoch;
        }
        k_os_pass<THREADS, ITEMS, ATOMIC_RANK, RB><<<dim3(grid), dim3(THREADS), 0, st>>>(b, (uint32_t)n, n_dev, p, passes, ghist, ghist_other, status, acc_base + (s.acc_flip ? acc_words : 0), acc_base + (s.acc_flip ? 0 : acc_words), (uint32_t)cap_groups, (uint32_t)acc_words,
                                                                         s.epoch & 0x3FFFFFFFu,
                                                                         s.err ? s.err : s.totals, s.totals + 64 + (s.acc_flip ? 1 : 0), s.totals + 64 + (s.acc_flip ? 0 : 1), bias, identity_vals ? 1 : 0,
                                                                         plan.hybrid ? plan.top : RB * p, plan.hybrid ? OS_TOP_ROW : p, plan.hybrid ? 1 : 0, (stampf && p == stamp_pass) ? stamps : nullptr);
        s.acc_flip ^= 1;
        ++s.stat_launches;
    }
    if (plan.hybrid) {
        if (RB != 9 || n_dev) return hipErrorInvalidValue;
        const OsSegSrc seg{ s.seg_pairs, s.seg_runs, plan.seg_rows, ghist_other };
        if (plan.segfeed && (!have_hist || !identity_vals || !seg.pairs || !seg.runs || seg.rows < 1u || seg.rows > SEGFEED_MAX_ROWS)) return hipErrorInvalidValue;      // only a producer's plan is segment-fed
        if (plan.segfeed) {
            if (plan.top <= 16) k_os_tail<256, true><<<dim3(OT_BINS), dim3(OT_THREADS), 0, st>>>(b, (uint32_t)n, ghist, bias, plan.top, os_tail_cap(s), s.fb_dev, s.err ? s.err : s.totals, seg);
            else k_os_tail<512, true><<<dim3(OT_BINS), dim3(OT_THREADS), 0, st>>>(b, (uint32_t)n, ghist, bias, plan.top, os_tail_cap(s), s.fb_dev, s.err ? s.err : s.totals, seg);
        }
        else if (plan.top <= 16) k_os_tail<256, false><<<dim3(OT_BINS), dim3(OT_THREADS), 0, st>>>(b, (uint32_t)n, ghist, bias, plan.top, os_tail_cap(s), s.fb_dev, s.err ? s.err : s.totals, seg);      // local digits of <= 8 bits
        else k_os_tail<512, false><<<dim3(OT_BINS), dim3(OT_THREADS), 0, st>>>(b, (uint32_t)n, ghist, bias, plan.top, os_tail_cap(s), s.fb_dev, s.err ? s.err : s.totals, seg);
        ++s.stat_launches; ++s.stat_hybrid;
    } else if (plan.top >= 0) {
        k_os_top_stats<<<dim3(1), dim3(OT_THREADS), 0, st>>>(ghist, os_tail_cap(s), s.fb_dev);
        ++s.stat_launches;
    }
    if (stampf && stamps) {   // tuning aid: dump per-tile wall-clock stamps (100 MHz) of one pass
        (void)hipStreamSynchronize(st);
        std::vector<u64> hs((size_t)tiles * 8);
        (void)hipMemcpy(hs.data(), stamps, hs.size() * 8, hipMemcpyDeviceToHost);
        FILE* f = fopen(stampf, "w");
        if (f) { for (uint32_t t = 0; t < tiles; ++t) { for (int k = 0; k < 6; ++k) fprintf(f, "%llu ", hs[t * 8 + k] - hs[0]); fprintf(f, "\n"); } fclose(f); }
        (void)hipFree(stamps);
    }
    return hipGetLastError();
}

// Digit width of a sort of `key_bits`-bit keys: 9-bit digits (512 bins) where they save a pass over 8-bit ones — 17-18 and 25-27 key bits, e.g. the
// depth keys of slowly moving (4D) splats, whose host-proven span is a little wider than 2^24; the tile shape needs a thread per bin.
int sort_plan_rb(const SortScratch& s, size_t n, int key_bits) {
    (void)n;
    if (s.rb_knob == 8 || s.rb_knob == 9) return (s.rb_knob == 9 && (s.shape_knob == 1 || s.shape_knob == 4)) ? 8 : s.rb_knob;      // test hook (the 256-thread shapes have no 512-bin form)
    if (s.shape_knob == 1 || s.shape_knob == 4) return 8;
    const int p8 = std::max(2, (key_bits + 7) / 8), p9 = std::max(2, (key_bits + 8) / 9);
    // (Beyond 27 bits both take four launches.  Preferring 9-bit digits there — their last digit is bits 27-31 only and is skipped on the device when
    // no key reaches 2^27 above the bias — was measured on the 4D sweep of BASELINE.json configs[3], whose bound is open-ended: 39.36 against 39.26 ms, nothing.)
    return p9 < p8 ? 9 : 8;
}
int sort_plan_passes(int key_bits, int rb) { return std::min(OS_MAX_PASSES, std::max(2, (key_bits + rb - 1) / rb)); }      // an even number of executed passes always exists (see os_schedule)

void sort_plan_hist(SortScratch& s, size_t n, int key_bits, uint32_t seg_rows) {
    const OsPlan p = os_plan(s, n, key_bits);
    s.hist_rb = sort_plan_rb(s, n, key_bits);
    s.hist_rows = p.rows; s.hist_top = p.top; s.hist_hybrid = p.hybrid;
    // segment-fed: a hybrid whose producer is the staged projection, where the knob allows it and the blocks and the run table hold that many segments
    s.hist_segfeed = p.hybrid && s.segfeed && seg_rows >= 1u && seg_rows <= SEGFEED_MAX_ROWS && s.seg_pairs && s.seg_runs &&
                     (size_t)seg_rows * SEGFEED_BLOCK <= s.seg_cap && (size_t)seg_rows * OS_MAX_BINS <= s.runs_cap;
    s.hist_seg_rows = s.hist_segfeed ? seg_rows : 0u;
}

hipError_t radix_sort_pairs(hipStream_t st, SortScratch& s, uint32_t* keys, uint32_t* vals, size_t n, const uint32_t* n_dev, int key_bits, bool have_hist, bool identity_vals) {
    if (n <= 1) { if (n == 1 && identity_vals) return hipMemsetAsync(vals, 0, 4, st); return hipSuccess; }      // radix_sort.hpp:260
    if (n >= (1ull << 32) - 1) return hipErrorInvalidValue;
    hipError_t e = sort_scratch_reserve(st, s, n);
    if (e != hipSuccess) return e;
    // the producer of the histograms (have_hist) counted digits of s.hist_rb bits: whoever set hist_bits chose it with sort_plan_rb
    const int rb = have_hist ? s.hist_rb : sort_plan_rb(s, n, key_bits);
    if (rb != 8 && rb != 9) return hipErrorInvalidValue;
    const int passes = sort_plan_passes(key_bits, rb);
    // the plan: the producer's (it counted the rows of that plan), or this call's own when k_os_hist is about to count
    OsPlan plan;
    if (have_hist) { plan.rows = s.hist_rows; plan.top = s.hist_top; plan.hybrid = s.hist_hybrid; plan.segfeed = s.hist_segfeed; plan.seg_rows = s.hist_seg_rows; }
    else if (!n_dev) plan = os_plan(s, n, key_bits);
    s.hist_rows = OS_MAX_PASSES; s.hist_top = -1; s.hist_hybrid = false; s.hist_segfeed = false; s.hist_seg_rows = 0;       // (of the pending histogram, which this sort consumes)
    if (plan.hybrid) return n_dev ? hipErrorInvalidValue : onesweep<512, 12, true, 9>(st, s, keys, vals, n, nullptr, passes, have_hist, identity_vals, plan);
    // 8192-key tiles of 512 threads x 16 keys for every size.  Rounds 2-3 ran sorts of <= 1.5M keys as 1024 x 8 (the same 12.7 us per pass alone at 10^6 keys;
    // 2-3 % more frames per second with the frame lanes overlapping, as the frame then was).  With this round's frame (staged tile lists: two launches fewer,
    // a longer projection kernel) the 512-thread form wins by 3 % at C2 — 0.0980-0.0984 against 0.1010-0.1017 ms/frame, three alternating runs each; 512 x 12:
    // 0.0983-0.0997; 512 x 8: 0.104; 256 x 16: 0.105 — and 1.4 % on the 4D set (0.1213 against 0.1231): a 16-wave workgroup finds a free CU later than an
    // 8-wave one beside the other lanes' kernels.  2048-key tiles are slower alone (20.3 us) and overlapped.
    // 512 bins: the large sorts use 512 x 12 (48 KB of keys and values + 16 KB of per-wave counters: still two workgroups per CU).
    int shape = s.shape_knob ? s.shape_knob : 5;
    (void)n;
    if (rb == 9 && shape == 5 && !s.shape_knob) shape = 6;
    const bool atomic_rank = s.rank_knob ? s.rank_knob == 2 : s.atomic_rank;
#define GS4D_OS8(T, I) (atomic_rank ? onesweep<T, I, true, 8>(st, s, keys, vals, n, n_dev, passes, have_hist, identity_vals, plan) : onesweep<T, I, false, 8>(st, s, keys, vals, n, n_dev, passes, have_hist, identity_vals, plan))
#define GS4D_OS(T, I) (rb == 9 ? (atomic_rank ? onesweep<T, I, true, 9>(st, s, keys, vals, n, n_dev, passes, have_hist, identity_vals, plan) : onesweep<T, I, false, 9>(st, s, keys, vals, n, n_dev, passes, have_hist, identity_vals, plan)) : GS4D_OS8(T, I))
    switch (shape) {
    case 1: return rb == 8 ? GS4D_OS8(256, 8) : hipErrorInvalidValue;
    case 2: return GS4D_OS(512, 8);
    case 3: return GS4D_OS(1024, 8);
    case 4: return rb == 8 ? GS4D_OS8(256, 16) : hipErrorInvalidValue;
    case 5: return GS4D_OS(512, 16);
    case 6: return GS4D_OS(512, 12);
    default: return GS4D_OS(512, 4);
    }
#undef GS4D_OS
#undef GS4D_OS8
}

} // namespace gs4d
