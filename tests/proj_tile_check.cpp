// Stand-alone check of the plain part of csrc/proj_tile.h: the integer maps of a wave's stage of projected records — where a lane puts its record,
// which piece of the wave's range a lane takes on a turn, and where that piece stands in the stage — as the device's put_record and store_staged
// call them.  Prints one line per group of cases and exits 0 when every case holds.
// tests/test_proj_tile_host.py builds it plainly and with AddressSanitizer + UndefinedBehaviorSanitizer (an executable of its own) and runs it.
#include "../4dgaussiansplatrendering_amd/csrc/proj_tile.h"
#include <cstdio>
#include <vector>

using namespace gs4d::proj_tile;

static int g_failed = 0, g_cases = 0;
static void expect(bool ok, const char* what, unsigned long long a = 0, unsigned long long b = 0) {
    ++g_cases;
    if (!ok) { ++g_failed; printf("FAILED %s (%llu, %llu)\n", what, a, b); }
}

// One round of a wave that holds `have` records, its stage at `pitch`: the lanes with a record put theirs (put_record), then all 64 lanes store
// (store_staged).  The stage is an array of slots that remember who wrote them; memory is the wave's range in bytes.
static void wave_round(uint32_t have, uint32_t pitch) {
    const uint32_t slots = WAVE * pitch;
    expect(stage_bytes(1, pitch) == slots * 16u && stage_bytes(8, pitch) == 8u * slots * 16u, "stage_bytes", have, pitch);
    std::vector<int> owner(slots, -1), piece_of(slots, -1);        // the record (lane) that wrote a slot, and which of its pieces
    bool disjoint = true;
    for (uint32_t r = 0; r < have; ++r) for (uint32_t k = 0; k < PIECES; ++k) {
        const uint32_t s = record_slot(r, pitch) + k;
        disjoint = disjoint && s < slots && owner[s] < 0;          // inside the wave's stage; no two records share a slot
        if (s < slots) { owner[s] = (int)r; piece_of[s] = (int)k; }
    }
    expect(disjoint, "no two records share a slot", have, pitch);

    std::vector<uint32_t> stored(PIECES * WAVE, 0);                 // per piece of a full wave's range: how often it was stored
    bool read_ok = true, to_ok = true, in_range = true;
    for (uint32_t lane = 0; lane < WAVE; ++lane) for (uint32_t t = 0; t < PIECES; ++t) {
        const uint32_t j = turn_piece(lane, t);
        in_range = in_range && j < PIECES * WAVE;
        if (j >= PIECES * have) continue;                           // (store_staged's guard)
        const uint32_t s = piece_slot(j, pitch);
        read_ok = read_ok && s < slots && owner[s] >= 0 && (uint32_t)owner[s] < have;            // every slot read was written by a lane with a record
        // piece j goes to byte 16 j of the wave's range: that is piece j % 4 of record j / 4, and the slot read holds exactly that
        to_ok = to_ok && s < slots && (uint32_t)owner[s] == j / PIECES && (uint32_t)piece_of[s] == j % PIECES && 16u * j == 64u * (uint32_t)owner[s] + 16u * (uint32_t)piece_of[s];
        ++stored[j];
    }
    bool exact = true;                                              // the pieces stored are exactly [0, 4 have), each once
    for (uint32_t j = 0; j < PIECES * WAVE; ++j) exact = exact && stored[j] == (j < PIECES * have ? 1u : 0u);
    expect(in_range, "a turn's piece lies in a full wave's range", have, pitch);
    expect(exact, "the pieces stored are [0, 4 have), each once", have, pitch);
    expect(read_ok, "every slot read was put by a lane with a record", have, pitch);
    expect(to_ok, "piece j is piece j % 4 of record j / 4, at byte 16 j", have, pitch);
}

int main() {
    expect(PIECES == 4 && WAVE == 64 && PITCH_DENSE == 4 && PITCH_ODD == 5 && (PITCH == PITCH_DENSE || PITCH == PITCH_ODD), "the constants");
    for (uint32_t pitch : { PITCH_DENSE, PITCH_ODD }) for (uint32_t have = 0; have <= WAVE; ++have) wave_round(have, pitch);
    printf("wave rounds: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // wave_have: the records of the wave at `first` below `end`, also where first + 64 wraps and where the wave lies past the end
    for (uint32_t first : { 0u, 64u, 4096u, 0xFFFFFF80u, 0xFFFFFFC0u }) for (uint32_t d : { 0u, 1u, 63u, 64u, 65u, 512u }) {
        const uint64_t end = (uint64_t)first + d;
        if (end > 0xFFFFFFFFull) continue;
        expect(wave_have(first, (uint32_t)end) == (d < 64u ? d : 64u), "wave_have", first, d);
        if (first >= d) expect(wave_have(first, first - d) == 0u, "wave_have past the end", first, d);
    }
    printf("wave_have: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
