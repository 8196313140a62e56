// lod_query_check — the text of gs4d_lod_cut's predicates (csrc/lod_query.h, what csrc/lod.hip evaluates on the device and the host library on the
// CPU) compiled stand-alone: tests/test_lod_host.py builds this with `g++ -O2 -std=c++17 -ffp-contract=off` (and once more with
// -fsanitize=address,undefined) and compares its output with gs4d_host_lod_cut, word for word.  Both sides are the same text, so this checks the
// flags and the compilers.  The buffers are allocated at exactly the sizes the definition demands, so the instrumented build also shows that nothing
// past node or parent word n - 1 is read, and no state byte of a parent word that is not a node.
//
//   lod_query_check N QUERY NODES PARENT CAPACITY DST CUT_INDEX STATE COUNT
//   lod_query_check refusals
// QUERY: the 112 bytes of a gs4d_lod_query.  NODES: N records of 24 float32.  PARENT: N uint32.  DST / CUT_INDEX: min(drawn, CAPACITY) records /
// uint32.  STATE: N bytes (0 STOP, 1 DESCEND, 2 DRAW).  COUNT: {drawn, written, tested, drawn_leaves}.  A query the call refuses: exit status 3.
// refusals: every GS4D_E_INVALID case of gs4d_lod_append and gs4d_lod_cut through the checks gs4d_api.hip makes before it queues anything — the query
// check of lod_query.h, and the scalar rule and the operand lists of lod_operands.h under check_operand_list — over a table of buffers of its own.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/gs4d.h"
#include "../4dgaussiansplatrendering_amd/csrc/lod_query.h"
#include "../4dgaussiansplatrendering_amd/csrc/lod_operands.h"
#include <map>

namespace lod = gs4d_lod;

static bool slurp(const char* path, void* to, size_t bytes) {
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::perror(path); return false; }
    const bool ok = bytes == 0 || std::fread(to, 1, bytes, in) == bytes;
    std::fclose(in);
    if (!ok) std::fprintf(stderr, "%s: too short\n", path);
    return ok;
}
static bool spill(const char* path, const void* from, size_t bytes) {
    FILE* f = std::fopen(path, "wb");
    if (!f) { std::perror(path); return false; }
    const bool ok = bytes == 0 || std::fwrite(from, 1, bytes, f) == bytes;
    return (std::fclose(f) == 0) && ok;
}

// ---- refusals ----
static std::map<uint32_t, gs4d::BufferFacts> g_bufs;      // name -> {live, bytes}; a name that is not here is unknown
static gs4d::BufferFacts lookup(uint32_t name) { auto it = g_bufs.find(name); return it == g_bufs.end() ? gs4d::BufferFacts{ false, 0 } : it->second; }
static int g_cases = 0, g_failed = 0;
static void expect(const char* what, bool refused, bool want) {
    ++g_cases;
    if (refused != want) { ++g_failed; std::printf("FAILED %s: %s\n", what, refused ? "refused" : "taken"); }
}
// whether gs4d_lod_append refuses: its numbers, then its buffers
static bool append_refused(uint32_t level, uint64_t m, uint32_t mg, uint64_t child_first, uint64_t c, uint32_t nodes, uint32_t parent, uint64_t first) {
    if (gs4d::lod_append_fault(m, mg != 0, child_first, c, first)) return true;
    gs4d::Operand op[gs4d::LOD_APPEND_OPERANDS];
    gs4d::lod_append_operands(op, level, m, mg, c, nodes, parent, first);
    return gs4d::check_operand_list(op, gs4d::LOD_APPEND_OPERANDS, lookup).fault != gs4d::OperandFault::None;
}
// whether gs4d_lod_cut refuses: its query, then its buffers
static bool cut_refused(uint32_t nodes, uint32_t parent, uint64_t n, const gs4d_lod_query* q, uint32_t dst, uint32_t index, uint32_t stats, uint32_t count) {
    if (!q || !lod::query_ok(*q, n)) return true;
    gs4d::Operand op[gs4d::LOD_CUT_OPERANDS];
    gs4d::lod_cut_operands(op, nodes, parent, n, dst, index, stats, count);
    return gs4d::check_operand_list(op, gs4d::LOD_CUT_OPERANDS, lookup).fault != gs4d::OperandFault::None;
}
static int refusals() {
    // buffers: 1 level (100 records), 2 member_group (300 words), 3 nodes (400 records), 4 parent (400 words), 5 destroyed, 6 dst (7 records),
    // 7 cut_index (9 words), 8 stats (400 rows), 9 count (16 bytes), 9999 unknown
    g_bufs = { { 1, { true, 100 * 96 } }, { 2, { true, 300 * 4 } }, { 3, { true, 400 * 96 } }, { 4, { true, 400 * 4 } }, { 5, { false, 1 << 20 } },
               { 6, { true, 7 * 96 } }, { 7, { true, 9 * 4 } }, { 8, { true, 400 * 16 } }, { 9, { true, 16 } } };
    // gs4d_lod_append(level, m, member_group, child_first, c, nodes, parent, first)
    expect("append: a level with its children", append_refused(1, 100, 2, 0, 300, 3, 4, 300), false);
    expect("append: the leaves", append_refused(1, 100, 0, 0, 0, 3, 4, 0), false);
    expect("append: child_first + c == first", append_refused(1, 100, 2, 100, 200, 3, 4, 300), false);
    expect("append: nothing to do", append_refused(1, 0, 0, 0, 0, 3, 4, 400), false);
    expect("append: child_first + c > first", append_refused(1, 100, 2, 1, 300, 3, 4, 300), true);
    expect("append: child_first > first", append_refused(1, 100, 2, 301, 0, 3, 4, 300), true);
    expect("append: child_first + c wraps", append_refused(1, 100, 2, 2, ~0ull, 3, 4, 300), true);
    expect("append: first + m > 0xFFFFFFFE", append_refused(1, 100, 0, 0, 0, 3, 4, 0xFFFFFFFEull - 99), true);
    expect("append: first + m wraps", append_refused(1, ~0ull, 0, 0, 0, 3, 4, 2), true);
    expect("append: c != 0 without member_group", append_refused(1, 100, 0, 0, 300, 3, 4, 300), true);
    const uint32_t good[4] = { 1, 2, 3, 4 };
    for (int at = 0; at < 4; ++at) {
        const uint32_t names[3] = { 5, 9999, 0 };               // destroyed, unknown, not given (member_group: the c != 0 rule)
        for (uint32_t bad : names) {
            uint32_t a[4] = { good[0], good[1], good[2], good[3] };
            a[at] = bad;
            expect("append: a buffer that is not live", append_refused(a[0], 100, a[1], 0, 300, a[2], a[3], 300), true);
        }
        for (int other = 0; other < at; ++other) {
            uint32_t a[4] = { good[0], good[1], good[2], good[3] };
            a[at] = a[other];
            expect("append: two arguments naming one buffer", append_refused(a[0], 100, a[1], 0, 300, a[2], a[3], 300), true);
        }
    }
    expect("append: level too short", append_refused(1, 101, 2, 0, 299, 3, 4, 299), true);
    expect("append: member_group too short", append_refused(1, 99, 2, 0, 301, 3, 4, 301), true);
    expect("append: nodes too short", append_refused(1, 100, 2, 0, 300, 3, 4, 301), true);
    g_bufs[3] = { true, 401 * 96 };
    expect("append: parent too short", append_refused(1, 100, 2, 0, 300, 3, 4, 301), true);
    g_bufs[3] = { true, 400 * 96 };
    std::printf("append: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // gs4d_lod_cut(nodes, parent, n, q, dst, cut_index, stats, count)
    gs4d_lod_query q;
    std::memset(&q, 0, sizeof(q));
    q.ratio = 0.5f; q.levels = 3; q.level_first[1] = 300; q.level_first[2] = 300; q.level_first[3] = 400;
    expect("cut: every output", cut_refused(3, 4, 400, &q, 6, 7, 8, 9), false);
    expect("cut: the count alone", cut_refused(3, 4, 400, &q, 0, 0, 0, 9), false);
    expect("cut: q == NULL", cut_refused(3, 4, 400, nullptr, 6, 7, 8, 9), true);
    { gs4d_lod_query b = q; b.levels = 0; expect("cut: levels 0", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.levels = 17; expect("cut: levels 17", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.levels = 16; for (int k = 3; k < 17; ++k) b.level_first[k] = 400; expect("cut: levels 16", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), false); }
    { gs4d_lod_query b = q; b.level_first[0] = 1; expect("cut: level_first[0] != 0", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.level_first[2] = 299; expect("cut: level_first decreases", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.level_first[3] = 399; expect("cut: level_first[levels] below n", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    expect("cut: level_first[levels] above n", cut_refused(3, 4, 399, &q, 6, 7, 8, 9), true);
    { gs4d_lod_query b = q; b.ratio = std::nanf(""); expect("cut: ratio NaN", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.ratio = -1e-30f; expect("cut: ratio below 0", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.ratio = INFINITY; expect("cut: ratio +inf", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), false); }
    { gs4d_lod_query b = q; b.ratio = 0.0f; expect("cut: ratio 0", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), false); }
    { gs4d_lod_query b = q; b.near_dist = INFINITY; expect("cut: near_dist +inf", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.near_dist = std::nanf(""); expect("cut: near_dist NaN", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.near_dist = -1.0f; expect("cut: near_dist below 0", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.near_dist = 3.0e38f; expect("cut: near_dist large", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), false); }
    { gs4d_lod_query b = q; b.flags = 1; expect("cut: flags", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    for (int r = 0; r < 3; ++r) { gs4d_lod_query b = q; b.reserved[r] = 1; expect("cut: reserved", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), true); }
    { gs4d_lod_query b = q; b.eye[0] = std::nanf(""); b.eye[1] = INFINITY; b.t = std::nanf(""); expect("cut: eye and t are data", cut_refused(3, 4, 400, &b, 6, 7, 8, 9), false); }
    { gs4d_lod_query b = q; b.levels = 1; b.level_first[1] = 0xFFFFFFFFu; g_bufs[10] = { true, ~(size_t)0 };
      expect("cut: n == 0xFFFFFFFF", cut_refused(10, 4, 0xFFFFFFFFull, &b, 0, 0, 0, 9), true); }
    const uint32_t names[6] = { 3, 4, 6, 7, 8, 9 };
    for (int at = 0; at < 6; ++at) {
        const bool optional = at >= 2 && at <= 4;
        const uint32_t bad[3] = { 5, 9999, 0 };
        for (uint32_t b : bad) {
            uint32_t a[6]; std::memcpy(a, names, sizeof(a));
            a[at] = b;
            expect("cut: a buffer that is not live, or not given", cut_refused(a[0], a[1], 400, &q, a[2], a[3], a[4], a[5]), !(b == 0 && optional));
        }
        for (int other = 0; other < at; ++other) {
            uint32_t a[6]; std::memcpy(a, names, sizeof(a));
            a[at] = a[other];
            expect("cut: two arguments naming one buffer", cut_refused(a[0], a[1], 400, &q, a[2], a[3], a[4], a[5]), true);
        }
    }
    const size_t full[4] = { 400 * 96, 400 * 4, 400 * 16, 16 };
    const uint32_t sized[4] = { 3, 4, 8, 9 };
    for (int k = 0; k < 4; ++k) {
        g_bufs[sized[k]].bytes = full[k] - 1;
        expect("cut: a buffer one byte short", cut_refused(3, 4, 400, &q, 6, 7, 8, 9), true);
        g_bufs[sized[k]].bytes = full[k];
    }
    g_bufs[6].bytes = 0; g_bufs[7].bytes = 3;                   // dst and cut_index hold what they hold: no slot, so nothing is written to them
    expect("cut: outputs without a slot", cut_refused(3, 4, 400, &q, 6, 7, 8, 9), false);
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "refusals") == 0) return refusals();
    if (argc != 10) { std::fprintf(stderr, "usage: lod_query_check N QUERY NODES PARENT CAPACITY DST CUT_INDEX STATE COUNT\n"); return 2; }
    const size_t n = (size_t)std::strtoull(argv[1], nullptr, 10), capacity = (size_t)std::strtoull(argv[5], nullptr, 10);
    gs4d_lod_query q;
    static_assert(sizeof(q) == 112, "the structure of include/gs4d.h");
    std::vector<float> rec(24 * n);
    std::vector<uint32_t> parent(n);
    if (!slurp(argv[2], &q, sizeof(q)) || !slurp(argv[3], rec.data(), 96 * n) || !slurp(argv[4], parent.data(), 4 * n)) return 2;
    if (!lod::query_ok(q, n)) return 3;
    const lod::View view = lod::view_of(q);
    std::vector<uint8_t> state(n, (uint8_t)lod::STOP);
    uint32_t tested = 0, drawn = 0, drawn_leaves = 0;
    for (int k = (int)q.levels - 1; k >= 0; --k) {
        const uint32_t next_first = q.level_first[k + 1];
        for (size_t i = q.level_first[k]; i < next_first; ++i) {
            const uint32_t p = parent[i];
            if (lod::is_child(p, next_first, (uint32_t)n) && state[p] != lod::DESCEND) continue;
            ++tested;
            const bool leaf = i < q.level_first[1];
            state[i] = lod::tested_state(leaf, !leaf && lod::fine(view, rec.data() + 24 * i));
        }
    }
    std::vector<float> dst;
    std::vector<uint32_t> index;
    for (size_t i = 0; i < n; ++i) {
        if (state[i] != lod::DRAW) continue;
        if (drawn < capacity) { dst.insert(dst.end(), rec.begin() + 24 * i, rec.begin() + 24 * (i + 1)); index.push_back((uint32_t)i); }
        if (i < q.level_first[1]) ++drawn_leaves;
        ++drawn;
    }
    const uint32_t count[4] = { drawn, (uint32_t)index.size(), tested, drawn_leaves };
    if (!spill(argv[6], dst.data(), 4 * dst.size()) || !spill(argv[7], index.data(), 4 * index.size()) || !spill(argv[8], state.data(), n) ||
        !spill(argv[9], count, sizeof(count))) return 2;
    return 0;
}
