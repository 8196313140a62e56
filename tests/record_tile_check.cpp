// Stand-alone check of the plain part of csrc/record_tile.h: the host loop that launches the record kernels in runs of workgroups, driven by a
// recording functor, and the integer maps of the staged tile — which piece a work item takes on a turn, and where that piece stands in the stage —
// as the device's store_staged and load_staged call them.  Prints one line per group of cases and exits 0 when every case holds.
// tests/test_record_tile_host.py builds it plainly and with AddressSanitizer + UndefinedBehaviorSanitizer (an executable of its own) and runs it.
#include "../4dgaussiansplatrendering_amd/csrc/record_tile.h"
#include <cstdio>
#include <utility>
#include <vector>

using namespace gs4d;

static int g_failed = 0, g_cases = 0;
static void expect(bool ok, const char* what, unsigned long long a = 0, unsigned long long b = 0) {
    ++g_cases;
    if (!ok) { ++g_failed; printf("FAILED %s (%llu, %llu)\n", what, a, b); }
}

// 1. the runs tile [0, groups) exactly and in order, none longer than max_grid and none empty
static void runs_tile(uint64_t groups, uint32_t max_grid) {
    std::vector<std::pair<uint64_t, uint32_t>> runs;
    const int e = launch_runs(groups, [&](uint64_t g0, uint32_t g) { runs.push_back({ g0, g }); return 0; }, max_grid);
    uint64_t next = 0;
    bool ok = e == 0;
    for (const auto& r : runs) { ok = ok && r.first == next && r.second >= 1 && r.second <= max_grid; next += r.second; }
    ok = ok && next == groups && runs.size() == (groups + max_grid - 1) / max_grid;
    expect(ok, "runs tile [0, groups)", groups, max_grid);
}
// the same, counted without storing the runs
static void runs_tile_counted(uint64_t groups, bool default_grid, uint32_t max_grid) {
    uint64_t next = 0, calls = 0;
    bool ok = true;
    auto rec = [&](uint64_t g0, uint32_t g) { ok = ok && g0 == next && g >= 1 && g <= max_grid; next += g; ++calls; return 0; };
    const int e = default_grid ? launch_runs(groups, rec) : launch_runs(groups, rec, max_grid);
    expect(ok && e == 0 && next == groups && calls == (groups + max_grid - 1) / max_grid, "runs tile [0, groups), counted", groups, max_grid);
}

// 3. the staged walk of a workgroup's tile of `slots` records (at most 256): with step 256 the workgroup's 256 threads walk the tile; with step 64
// each of its four waves walks the records from its first one, 64 * wave, as a tile of its own in its own part of the stage (transform_selected.hip)
static void staged_walk(uint32_t slots, uint32_t step) {
    std::vector<char> put(slots * RECORD_PITCH, 0);      // the slots of the stage that put_record wrote: six pieces from r * RECORD_PITCH
    for (uint32_t r = 0; r < slots; ++r) for (uint32_t k = 0; k < RECORD_PIECES; ++k) put[r * RECORD_PITCH + k] = 1;
    std::vector<uint32_t> visits(slots * RECORD_PIECES, 0);
    bool ok = true;
    for (uint32_t first = 0; first < slots; first += step) {                             // (a wave past the tile's end has nothing selected and returns)
        const uint32_t pieces = tile_slots(slots - first, step) * RECORD_PIECES;
        for (uint32_t item = 0; item < step; ++item) for (uint32_t u = 0; u < RECORD_PIECES; ++u) {
            const uint32_t j = turn_piece(item, u, step);
            if (j >= pieces) continue;                   // (store_staged's guard)
            const uint32_t piece = first * RECORD_PIECES + j, s = first * RECORD_PITCH + piece_slot(j);
            ++visits[piece];
            ok = ok && s < slots * RECORD_PITCH && put[s];
            ok = ok && s / RECORD_PITCH == piece / RECORD_PIECES && s % RECORD_PITCH == piece % RECORD_PIECES;      // piece % 6 of record piece / 6
        }
    }
    for (uint32_t v : visits) ok = ok && v == 1;
    expect(ok, "staged walk", slots, step);
}

// 4. pose's spans: launch_runs over the tiles in spans of at most max_grid * walk, a grid of walk_grid(span, walk) workgroups per span, workgroup b
// of it taking the tiles t0 + b, + grid, ... below t0 + span
static void pose_spans(uint32_t tiles, uint32_t walk, uint32_t max_grid) {
    std::vector<uint32_t> visits(tiles, 0);
    bool ok = true;
    const int e = launch_runs(tiles, [&](uint64_t t0, uint32_t span) {
        const uint32_t grid = walk_grid(span, walk), t1 = (uint32_t)t0 + span;
        ok = ok && grid >= 1 && grid <= max_grid;
        for (uint32_t b = 0; b < grid; ++b) {
            uint32_t taken = 0;
            for (uint64_t t = t0 + b; t < t1; t += grid) { ++visits[t]; ++taken; }
            ok = ok && taken >= 1 && taken <= walk;
        }
        return 0;
    }, max_grid * walk);
    for (uint32_t t = 0; t < tiles; ++t) ok = ok && visits[t] == 1;
    expect(ok && e == 0, "pose spans", tiles, walk);
}

int main() {
    for (uint32_t mg : { 1u, 4u }) for (uint64_t groups : { (uint64_t)0, (uint64_t)1, (uint64_t)mg - 1, (uint64_t)mg, (uint64_t)mg + 1, (uint64_t)3 * mg + 1 }) runs_tile(groups, mg);
    runs_tile_counted(0xFFFFFFFFull, false, 1u << 22);
    runs_tile_counted(0xFFFFFFFFull, false, 0xFFFFFFFFu);
    runs_tile_counted(0x100000000ull, true, RECORD_MAX_GRID);
    runs_tile_counted(0x100000000ull, false, 0xFFFFFFFFu);
    expect(RECORD_MAX_GRID == 1u << 22, "the shipped max_grid");
    printf("runs: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // 2. an error returned by the k-th call ends the walk after exactly k calls, and is the value returned
    for (uint32_t mg : { 1u, 4u }) for (int k = 1; k <= 4; ++k) {
        int calls = 0;
        const int e = launch_runs((uint64_t)4 * mg, [&](uint64_t, uint32_t) { return ++calls == k ? 700 + k : 0; }, mg);
        expect(calls == k && e == 700 + k, "an error ends the walk", (unsigned long long)k, mg);
    }
    {   int calls = 0;
        const int e = launch_runs(0x100000000ull, [&](uint64_t, uint32_t) { return ++calls == 3 ? -5 : 0; });
        expect(calls == 3 && e == -5, "an error ends the walk, default max_grid"); }
    printf("errors: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    for (uint32_t slots : { 1u, 63u, 64u, 65u, 255u, 256u }) for (uint32_t step : { 256u, 64u })
        staged_walk(slots, step);
    for (uint32_t left : { 1u, 255u, 256u, 257u, 0xFFFFFFFFu }) expect(tile_slots(left, 256) == (left < 256 ? left : 256), "tile_slots", left);
    expect(tile_slots(0x100000000ull, 256) == 256, "tile_slots past 32 bits");
    printf("staged walk: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    for (uint32_t walk : { 1u, 4u }) for (uint32_t mg : { 1u, 3u }) for (uint32_t tiles : { 1u, 2u, 3u, 4u, 5u, 11u, 12u, 13u, 40u, 41u }) pose_spans(tiles, walk, mg);
    for (uint32_t walk : { 1u, 4u }) pose_spans((1u << 24), walk, RECORD_MAX_GRID);      // n = 0xFFFFFFFF: 2^24 tiles, four launches at walk 1
    printf("pose spans: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
