// merge.hip — gs4d_cell_labels and gs4d_merge_records (include/gs4d.h): a label per record from a 4D cell grid, and one
// moment-matched record per group of members with one label.  The arithmetic is the text of merge_record.h, which the host definitions compile too;
// this file is built with the flags of preprocess.hip (round to nearest, no contraction, correctly rounded division and square root).
//
// gs4d_cell_labels is one launch of one thread per record (k_cell_labels): one 16-byte load, one 4-byte store.
//
// gs4d_merge_records is a segmented reduction behind a sort, on one stream; no workgroup ever waits for another (kernel boundaries are the only
// dependencies):
//   k_merge_keys     one thread per record: the table row first (16 bytes, through keep_row), then the label, then the record's six 16-byte pieces;
//                    key = the label of a member, GS4D_ID_NONE otherwise;
//   the sort         radix_sort_pairs of the identity by key, 32 bits, stable (sort.hip): non-members go to the end, every run of equal keys is in
//                    ascending record index — the order the definition adds a group's members in;
//   k_merge_count    one workgroup per tile of MERGE_TILE sorted keys: the run heads of the tile (a key below GS4D_ID_NONE that differs from the key
//                    in front of it) counted with wave ballots, ONE word per tile;
//   k_merge_scan     one workgroup: exclusive sum of the tile counts, in place; one thread finds where the non-members begin (a bisection of the
//                    sorted keys) and writes the caller's gs4d_merge_count and the state block {groups, members};
//   k_merge_heads    one workgroup per tile: the heads again, their numbers from the tile's base, ballot prefixes and the wave offsets:
//                    start[g] = sorted slot of group g's first member, member_group[index] = the group of every member, GS4D_ID_NONE otherwise;
//   k_merge_groups   one sub-group of 8 lanes per group (8 groups per wave, 32 per workgroup).  Lane l walks members l, l + 8, ... of the run, gathers
//                    each one's six 16-byte pieces, recomputes its mass with the shared text and adds it into its slot of 18 doubles, which stay
//                    in registers.  A butterfly of __shfl_xor over lane distances 1, 2 and 4 is the definition's tree in every lane.  Lanes 0..5 then
//                    each store one 16-byte piece of the record (a wave writes 768 contiguous bytes), lane 6 the gs4d_merge_group row.  No LDS, no
//                    atomics, no private memory.  The grid covers n / 32 workgroups, since the group count is known on the device only; sub-groups
//                    past the count leave at once.  A group of a million members is walked by its eight lanes alone.
// Scratch (the lane's, merge_scratch_words()): keys, sorted indices and run starts of n words each, the tile counts and the state block.  All byte
// offsets are 64-bit.  No slot >= cap of dst or groups is written; records, labels and table are only read, and only rows < n.
#include "gs4d_internal.h"
#include "merge_record.h"
#include "record_tile.h"      // f32x4

namespace gs4d {

namespace mg = gs4d_merge;
constexpr uint32_t MG_THREADS = 256, MG_WAVES = MG_THREADS / 64, MG_ROUNDS = MERGE_TILE / MG_THREADS;
constexpr uint32_t MG_SUB = 8;                          // lanes of a sub-group: the slots of the definition
constexpr uint32_t MG_GROUPS_PER_WG = MG_THREADS / MG_SUB;
static_assert(MG_SUB == (uint32_t)mg::SLOTS, "one lane per slot");
static_assert(MG_ROUNDS * MG_WAVES <= 64 && MERGE_TILE % MG_THREADS == 0, "one wave scans the (round, wave) counts of a tile");
static_assert(sizeof(gs4d_merge_group) == sizeof(uint4) && sizeof(gs4d_merge_count) == sizeof(uint4) && sizeof(gs4d_cell_grid) == 64, "the structures of gs4d.h");

// ---- gs4d_cell_labels ----
__global__ __launch_bounds__(MG_THREADS) void k_cell_labels(const f32x4* __restrict__ rec, uint32_t n, gs4d_cell_grid g, uint32_t* __restrict__ labels) {
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    const f32x4 v = rec[i * 6u];
    const float p[4] = { v.x, v.y, v.z, v.w };
    labels[i] = mg::cell_label(g.lo, g.edge, g.dims, p);
}

hipError_t launch_cell_labels(hipStream_t st, const void* records, size_t n, const gs4d_cell_grid& grid, uint32_t* labels) {
    if (!n) return hipSuccess;
    if (n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    k_cell_labels<<<dim3((uint32_t)((n + MG_THREADS - 1) / MG_THREADS)), dim3(MG_THREADS), 0, st>>>((const f32x4*)records, (uint32_t)n, grid, labels);
    return hipGetLastError();
}

// ---- gs4d_merge_records ----
__device__ __forceinline__ void load_record(const f32x4* __restrict__ rec, uint64_t i, float r[24]) {
    const f32x4* const p = rec + i * 6u;
#pragma unroll
    for (uint32_t k = 0; k < 6u; ++k) { const f32x4 v = p[k]; r[4 * k] = v.x; r[4 * k + 1] = v.y; r[4 * k + 2] = v.z; r[4 * k + 3] = v.w; }
}

__global__ __launch_bounds__(MG_THREADS) void k_merge_keys(const f32x4* __restrict__ rec, uint32_t n, const uint32_t* __restrict__ labels,
                                                           const uint4* __restrict__ stats, KeepRule rule, uint32_t* __restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t key = mg::NONE;
    if (!stats || keep_row(stats[i], rule)) {
        const uint32_t label = labels[i];
        if (label != mg::NONE) {
            float r[24], a;
            load_record(rec, i, r);
            if (mg::member_mass(r, a)) key = label;
        }
    }
    keys[i] = key;
}

// whether sorted slot s of round r of a tile starts a group (thread t looks at slot tile0 + r * MG_THREADS + t: ascending (round, wave, lane) is
// ascending slot), and the slot's key
__device__ __forceinline__ bool run_head(const uint32_t* __restrict__ keys, uint64_t s, uint64_t n, uint32_t& key) {
    key = mg::NONE;
    if (s >= n) return false;
    key = keys[s];
    return key != mg::NONE && (s == 0u || keys[s - 1u] != key);
}

__global__ __launch_bounds__(MG_THREADS) void k_merge_count(const uint32_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wave_total[MG_WAVES];
    const uint64_t tile0 = (uint64_t)blockIdx.x * MERGE_TILE;
    uint32_t mine = 0;
#pragma unroll
    for (uint32_t r = 0; r < MG_ROUNDS; ++r) {
        uint32_t key;
        mine += (uint32_t)__popcll(__ballot(run_head(keys, tile0 + r * MG_THREADS + threadIdx.x, n, key)));      // wave-uniform
    }
    if ((threadIdx.x & 63u) == 0u) wave_total[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) { uint32_t s = 0; for (uint32_t w = 0; w < MG_WAVES; ++w) s += wave_total[w]; counts[blockIdx.x] = s; }
}

// counts[0 .. ntiles) -> exclusive sums, in place; *count = {groups, min(groups, cap), members, n - members}; state = {groups, members}.
// One workgroup of 1024 threads walks the array in rounds of 1024 words (10^7 records: 5 rounds).
__global__ __launch_bounds__(1024) void k_merge_scan(uint32_t* __restrict__ counts, uint32_t ntiles, const uint32_t* __restrict__ keys, uint32_t n, uint32_t cap,
                                                     uint4* __restrict__ count, uint32_t* __restrict__ state) {
    __shared__ uint32_t wave_sum[16];
    __shared__ uint32_t carry_s;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0u) carry_s = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < ntiles; base += 1024u) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < ntiles ? counts[i] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v, lane);
        if (lane == 63u) wave_sum[wave] = incl;
        const uint32_t carry = carry_s;
        __syncthreads();
        uint32_t before = carry;
        for (uint32_t w = 0; w < wave; ++w) before += wave_sum[w];
        if (i < ntiles) counts[i] = before + incl - v;
        if (threadIdx.x == 1023u) carry_s = before + incl;      // (everybody took the old carry before the barrier above)
        __syncthreads();
    }
    if (threadIdx.x == 0u) {
        uint32_t lo = 0u, hi = n;                               // the first slot whose key is GS4D_ID_NONE: keys[lo - 1] < NONE <= keys[hi]
        while (lo < hi) { const uint32_t mid = lo + (hi - lo) / 2u; if (keys[mid] != mg::NONE) lo = mid + 1u; else hi = mid; }
        const uint32_t groups = carry_s, members = lo;
        *count = make_uint4(groups, groups < cap ? groups : cap, members, n - members);
        state[0] = groups; state[1] = members;
    }
}

__global__ __launch_bounds__(MG_THREADS) void k_merge_heads(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ index, uint64_t n,
                                                            const uint32_t* __restrict__ bases, uint32_t* __restrict__ start, uint32_t* __restrict__ member_group) {
    __shared__ uint32_t part[64];                               // heads of (round, wave), then their exclusive sums
    const uint64_t tile0 = (uint64_t)blockIdx.x * MERGE_TILE;
    const uint32_t base = bases[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    bool head[MG_ROUNDS];
    uint32_t key[MG_ROUNDS];
    uint64_t mask[MG_ROUNDS];
#pragma unroll
    for (uint32_t r = 0; r < MG_ROUNDS; ++r) {
        head[r] = run_head(keys, tile0 + r * MG_THREADS + threadIdx.x, n, key[r]);
        mask[r] = __ballot(head[r]);
        if (lane == 0u) part[r * MG_WAVES + wave] = (uint32_t)__popcll(mask[r]);
    }
    __syncthreads();
    if (threadIdx.x < 64u) {
        const uint32_t v = threadIdx.x < MG_ROUNDS * MG_WAVES ? part[threadIdx.x] : 0u;
        const uint32_t incl = wave_incl_scan_u32(v, lane);
        part[threadIdx.x] = incl - v;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < MG_ROUNDS; ++r) {
        const uint64_t s = tile0 + r * MG_THREADS + threadIdx.x;
        if (s >= n) continue;
        // heads at or in front of s, all tiles: s belongs to the group whose number is one less (a member has a head at or in front of it)
        const uint32_t upto = base + part[r * MG_WAVES + wave] + (uint32_t)__popcll(mask[r] & ((2ull << lane) - 1ull));
        if (head[r]) start[upto - 1u] = (uint32_t)s;
        if (member_group) member_group[index[s]] = key[r] != mg::NONE ? upto - 1u : mg::NONE;
    }
}

// a double from the lane `lane ^ d` of the wave
__device__ __forceinline__ double xor_lane(double v, int d) { return __shfl_xor(v, d, 64); }

__global__ __launch_bounds__(MG_THREADS) void k_merge_groups(const f32x4* __restrict__ rec, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ index,
                                                             const uint32_t* __restrict__ start, const uint32_t* __restrict__ state, float alpha_max, uint32_t cap,
                                                             f32x4* __restrict__ dst, uint4* __restrict__ rows) {
    const uint32_t groups = state[0], members = state[1];
    const uint32_t written = groups < cap ? groups : cap;
    const uint64_t g = ((uint64_t)blockIdx.x * MG_THREADS + threadIdx.x) / MG_SUB;
    const uint32_t l = threadIdx.x & (MG_SUB - 1u);
    const bool live = g < written;                             // (the same in all eight lanes of a sub-group)
    uint32_t first = 0u, end = 0u;
    if (live) { first = start[g]; end = g + 1u < groups ? start[g + 1u] : members; }
    const uint32_t size = end - first;
    float origin[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    float out[24];
#pragma unroll
    for (int w = 0; w < 24; ++w) out[w] = 0.0f;
    mg::Sums s;
    mg::clear(s);
    if (size == 1u) {
        load_record(rec, index[first], out);                    // a group of one member: its 24 words as they are
    } else if (size > 1u) {
        const f32x4 c = rec[(uint64_t)index[first] * 6u];
        origin[0] = c.x; origin[1] = c.y; origin[2] = c.z; origin[3] = c.w;
        for (uint64_t k = (uint64_t)first + l; k < end; k += MG_SUB) {
            float r[24], a;
            load_record(rec, index[k], r);
            (void)mg::member_mass(r, a);                        // the mass the key kernel found finite and > 0
            mg::add_member(s, origin, a, r);
        }
    }
    // every lane of the wave takes part in the butterfly; the lanes of a sub-group without a group exchange zeros
#pragma unroll
    for (int d = 1; d < (int)MG_SUB; d <<= 1) {
        mg::Sums o;
        o.w = xor_lane(s.w, d);
#pragma unroll
        for (int r = 0; r < 4; ++r) o.m[r] = xor_lane(s.m[r], d);
#pragma unroll
        for (int e = 0; e < 10; ++e) o.q[e] = xor_lane(s.q[e], d);
#pragma unroll
        for (int j = 0; j < 3; ++j) o.c[j] = xor_lane(s.c[j], d);
        mg::join(s, o);
    }
    if (!live) return;
    if (size > 1u) mg::finish(s, origin, alpha_max, out);
    if (l < 6u) {
        f32x4 v = f32x4{ out[0], out[1], out[2], out[3] };
#pragma unroll
        for (uint32_t k = 1; k < 6u; ++k) if (l == k) v = f32x4{ out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3] };
        dst[g * 6u + l] = v;
    }
    if (l == 6u && rows) rows[g] = make_uint4(keys[first], size, index[first], 0u);
}

__global__ void k_merge_empty(uint4* __restrict__ count) { *count = make_uint4(0u, 0u, 0u, 0u); }

// the run starts of n sorted keys (gs4d_internal.h): k_merge_count, k_merge_scan and k_merge_heads, which gs4d_merge_rows (merge_rows.hip) runs too
hipError_t launch_merge_run_starts(hipStream_t st, const uint32_t* keys, const uint32_t* index, size_t n, uint32_t* counts, uint32_t cap,
                                   gs4d_merge_count* count, uint32_t* state, uint32_t* start, uint32_t* member_group) {
    const uint32_t ntiles = (uint32_t)merge_tiles(n);
    k_merge_count<<<dim3(ntiles), dim3(MG_THREADS), 0, st>>>(keys, (uint64_t)n, counts);
    k_merge_scan<<<dim3(1), dim3(1024), 0, st>>>(counts, ntiles, keys, (uint32_t)n, cap, (uint4*)count, state);
    k_merge_heads<<<dim3(ntiles), dim3(MG_THREADS), 0, st>>>(keys, index, (uint64_t)n, counts, start, member_group);
    return hipGetLastError();
}

hipError_t launch_merge_records(hipStream_t st, SortScratch& sort, const void* records, size_t n, const uint32_t* labels, float alpha_max,
                                const gs4d_record_stat* stats, const KeepRule& rule, uint32_t* scratch, void* dst, gs4d_merge_group* groups,
                                uint32_t* member_group, uint32_t cap, gs4d_merge_count* count) {
    static_assert(sizeof(gs4d_record_stat) == sizeof(uint4), "a statistics row is one uint4");
    if (n >= 0xFFFFFFFFull) return hipErrorInvalidValue;       // (the sort takes 2^32 - 2 keys at most)
    if (!n) { k_merge_empty<<<dim3(1), dim3(1), 0, st>>>((uint4*)count); return hipGetLastError(); }
    // the scratch, in the order of merge_scratch_words(): keys, sorted indices, run starts (n words each, rounded up to 16 bytes), tile counts, state
    const size_t n4 = (n + 3) & ~(size_t)3;
    const uint32_t ntiles = (uint32_t)merge_tiles(n);
    uint32_t* const keys = scratch;
    uint32_t* const index = keys + n4;
    uint32_t* const start = index + n4;
    uint32_t* const counts = start + n4;
    uint32_t* const state = counts + ((ntiles + 3u) & ~3u);
    const uint32_t per_record = (uint32_t)((n + MG_THREADS - 1) / MG_THREADS);
    hipError_t e;
    k_merge_keys<<<dim3(per_record), dim3(MG_THREADS), 0, st>>>((const f32x4*)records, (uint32_t)n, labels, (const uint4*)stats, rule, keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = radix_sort_pairs(st, sort, keys, index, n, nullptr, 32, false, true)) != hipSuccess) return e;
    if ((e = launch_merge_run_starts(st, keys, index, n, counts, cap, count, state, start, member_group)) != hipSuccess) return e;
    if (cap) {
        const uint64_t most = n < cap ? n : cap;                // groups that can be written
        k_merge_groups<<<dim3((uint32_t)((most + MG_GROUPS_PER_WG - 1) / MG_GROUPS_PER_WG)), dim3(MG_THREADS), 0, st>>>(
            (const f32x4*)records, keys, index, start, state, alpha_max, cap, (f32x4*)dst, (uint4*)groups);
    }
    return hipGetLastError();
}

} // namespace gs4d
