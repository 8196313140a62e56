// merge_rows_check — the text of gs4d_merge_rows' definition (csrc/merge_rows_record.h, whose word functions csrc/merge_rows.hip evaluates on the
// device and whose loop is gs4d_host_merge_rows) compiled stand-alone: tests/test_merge_rows_host.py builds this with
// `g++ -O2 -std=c++17 -ffp-contract=off` (and once more with -fsanitize=address,undefined) and compares its output with gs4d_host_merge_rows, word
// for word.  Both sides are the same text, so this checks the flags and the compilers.  The buffers are allocated at exactly the sizes the definition
// demands, so the instrumented build also shows that nothing past record, group word or row n - 1 is read, nothing past word width - 1 of a row,
// and no row of dst at or beyond the capacity is written.
//
//   merge_rows_check N STRIDE WIDTH WEIGHTED DST_FIRST CAPACITY RECORDS MEMBER_GROUP ROWS DST_IN DST_OUT COUNT
//   merge_rows_check refusals
// RECORDS: N records of 24 float32 (read iff WEIGHTED is 1).  MEMBER_GROUP: N uint32.  ROWS: N rows of STRIDE bytes.  DST_IN / DST_OUT: CAPACITY rows
// of STRIDE bytes, before and after.  COUNT: {groups, written, members, left_out}.  A query the call refuses: exit status 3.
// refusals: every GS4D_E_INVALID case of gs4d_merge_rows and gs4d_copy_rows through the checks gs4d_api.hip makes before it queues anything — the
// scalar rules and the operand lists of rows_operands.h under check_operand_list — over a table of buffers of its own.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "../include/gs4d.h"
#include "../4dgaussiansplatrendering_amd/csrc/merge_rows_record.h"
#include "../4dgaussiansplatrendering_amd/csrc/rows_operands.h"

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
// whether gs4d_merge_rows refuses: its numbers, then its buffers
static bool merge_refused(uint32_t data, uint64_t n, uint32_t mg, uint32_t rows, const gs4d_rows_query* q, uint32_t dst, uint64_t dst_first, uint32_t count) {
    const gs4d_rows_query v = q ? *q : gs4d_rows_query{ 0, 0, 0, 0 };
    const bool scalar = gs4d::merge_rows_fault(q != nullptr, v.stride, v.width, v.flags, v.reserved, n, dst_first) != nullptr;
    // the definition's own check agrees with the call's
    if (q && n <= 0xFFFFFFFEull && dst_first <= 0xFFFFFFFEull && scalar == gs4d_rows::query_ok(v.stride, v.width, v.flags, v.reserved)) { ++g_failed; std::printf("FAILED: query_ok and merge_rows_fault disagree\n"); }
    if (scalar) return true;
    gs4d::Operand op[gs4d::MERGE_ROWS_OPERANDS];
    gs4d::merge_rows_operands(op, data, n, mg, rows, v.stride, dst, count);
    return gs4d::check_operand_list(op, gs4d::MERGE_ROWS_OPERANDS, lookup).fault != gs4d::OperandFault::None;
}
static bool copy_refused(uint32_t src, uint64_t src_first, uint64_t m, uint64_t stride, uint32_t dst, uint64_t dst_first) {
    if (gs4d::copy_rows_fault(src_first, m, stride, dst_first)) return true;
    gs4d::Operand op[gs4d::COPY_ROWS_OPERANDS];
    gs4d::copy_rows_operands(op, src, src_first, m, stride, dst, dst_first);
    return gs4d::check_operand_list(op, gs4d::COPY_ROWS_OPERANDS, lookup).fault != gs4d::OperandFault::None;
}
static int refusals() {
    // buffers: 1 data (100 records), 2 member_group (100 words), 3 rows (100 rows of 48 bytes), 4 dst (7 rows of 48 bytes), 5 destroyed,
    // 6 count (16 bytes), 9999 unknown
    g_bufs = { { 1, { true, 100 * 96 } }, { 2, { true, 100 * 4 } }, { 3, { true, 100 * 48 } }, { 4, { true, 7 * 48 } }, { 5, { false, 1 << 20 } }, { 6, { true, 16 } } };
    const gs4d_rows_query q{ 48, 12, 0, 0 };
    // gs4d_merge_rows(data, n, member_group, rows, q, dst, dst_first, count)
    expect("merge: weighted", merge_refused(1, 100, 2, 3, &q, 4, 0, 6), false);
    expect("merge: unit weights", merge_refused(0, 100, 2, 3, &q, 4, 0, 6), false);
    expect("merge: n == 0", merge_refused(1, 0, 2, 3, &q, 4, 0, 6), false);
    expect("merge: dst_first past the capacity", merge_refused(1, 100, 2, 3, &q, 4, 0xFFFFFFFEull, 6), false);
    expect("merge: q == NULL", merge_refused(1, 100, 2, 3, nullptr, 4, 0, 6), true);
    const uint32_t bad_strides[] = { 0, 8, 24, 47, 49, 1040, 2048, 0xFFFFFFF0u };
    for (uint32_t s : bad_strides) { gs4d_rows_query b = q; b.stride = s; b.width = 1; expect("merge: a stride that breaks the rule", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), true); }
    { gs4d_rows_query b = q; b.stride = 16; b.width = 4; g_bufs[3].bytes = 100 * 16; expect("merge: stride 16", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), false); }
    { gs4d_rows_query b = q; b.stride = 1024; b.width = 256; g_bufs[3].bytes = 100 * 1024; expect("merge: stride 1024", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), false); }
    g_bufs[3].bytes = 100 * 48;
    { gs4d_rows_query b = q; b.width = 0; expect("merge: width 0", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), true); }
    { gs4d_rows_query b = q; b.width = 13; expect("merge: 4 width > stride", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), true); }
    { gs4d_rows_query b = q; b.width = 0x40000003u; expect("merge: 4 width wraps", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), true); }
    { gs4d_rows_query b = q; b.width = 1; expect("merge: width 1", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), false); }
    { gs4d_rows_query b = q; b.flags = 1; expect("merge: flags", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), true); }
    { gs4d_rows_query b = q; b.reserved = 0x80000000u; expect("merge: reserved", merge_refused(1, 100, 2, 3, &b, 4, 0, 6), true); }
    g_bufs[10] = { true, ~(size_t)0 }; g_bufs[11] = { true, ~(size_t)0 }; g_bufs[12] = { true, ~(size_t)0 };
    expect("merge: n == 0xFFFFFFFE", merge_refused(10, 0xFFFFFFFEull, 11, 12, &q, 4, 0, 6), false);
    expect("merge: n == 0xFFFFFFFF", merge_refused(10, 0xFFFFFFFFull, 11, 12, &q, 4, 0, 6), true);
    expect("merge: dst_first == 0xFFFFFFFF", merge_refused(1, 100, 2, 3, &q, 4, 0xFFFFFFFFull, 6), true);
    expect("merge: dst_first == 2^32", merge_refused(1, 100, 2, 3, &q, 4, 1ull << 32, 6), true);
    const uint32_t names[5] = { 1, 2, 3, 4, 6 };
    for (int at = 0; at < 5; ++at) {
        const uint32_t bad[3] = { 5, 9999, 0 };
        for (uint32_t b : bad) {
            uint32_t a[5]; std::memcpy(a, names, sizeof(a));
            a[at] = b;
            expect("merge: a buffer that is not live, or not given", merge_refused(a[0], 100, a[1], a[2], &q, a[3], 0, a[4]), !(b == 0 && at == 0));
        }
        for (int other = 0; other < at; ++other) {
            uint32_t a[5]; std::memcpy(a, names, sizeof(a));
            a[at] = a[other];
            expect("merge: two arguments naming one buffer", merge_refused(a[0], 100, a[1], a[2], &q, a[3], 0, a[4]), true);
        }
    }
    const size_t full[4] = { 100 * 96, 100 * 4, 100 * 48, 16 };
    const uint32_t sized[4] = { 1, 2, 3, 6 };
    for (int k = 0; k < 4; ++k) {
        g_bufs[sized[k]].bytes = full[k] - 1;
        expect("merge: a buffer one byte short", merge_refused(1, 100, 2, 3, &q, 4, 0, 6), true);
        g_bufs[sized[k]].bytes = full[k];
    }
    g_bufs[1].bytes = 0;
    expect("merge: data too short does not matter when it is not given", merge_refused(0, 100, 2, 3, &q, 4, 0, 6), false);
    g_bufs[1].bytes = full[0];
    g_bufs[4].bytes = 47;                                       // dst holds what it holds: no row, so nothing is written to it
    expect("merge: a dst without a row", merge_refused(1, 100, 2, 3, &q, 4, 0, 6), false);
    g_bufs[4].bytes = 7 * 48;
    std::printf("merge: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // gs4d_copy_rows(src, src_first, m, stride, dst, dst_first)
    expect("copy: rows 93 .. 99 to rows 0 .. 6", copy_refused(3, 93, 7, 48, 4, 0), false);
    expect("copy: nothing to do", copy_refused(3, 100, 0, 48, 4, 7), false);
    expect("copy: src == dst", copy_refused(3, 0, 1, 48, 3, 50), true);
    expect("copy: src too short", copy_refused(3, 94, 7, 48, 4, 0), true);
    expect("copy: dst too short", copy_refused(3, 0, 7, 48, 4, 1), true);
    expect("copy: m == 0 past the end of dst", copy_refused(3, 0, 0, 48, 4, 8), true);
    for (uint32_t s : bad_strides) expect("copy: a stride that breaks the rule", copy_refused(3, 0, 1, s, 4, 0), true);
    expect("copy: m above 2^32 - 1", copy_refused(10, 0, 1ull << 32, 16, 11, 0), true);
    expect("copy: m == 2^32 - 1", copy_refused(10, 0, 0xFFFFFFFFull, 16, 11, 0), false);
    expect("copy: src_first above 2^32 - 1", copy_refused(10, 1ull << 32, 1, 16, 11, 0), true);
    expect("copy: dst_first above 2^32 - 1", copy_refused(10, 0, 1, 16, 11, ~0ull), true);
    for (uint32_t b : { 5u, 9999u, 0u }) {
        expect("copy: src not live", copy_refused(b, 0, 1, 48, 4, 0), true);
        expect("copy: dst not live", copy_refused(3, 0, 1, 48, b, 0), true);
    }
    std::printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "refusals") == 0) return refusals();
    if (argc != 13) { std::fprintf(stderr, "usage: merge_rows_check N STRIDE WIDTH WEIGHTED DST_FIRST CAPACITY RECORDS MEMBER_GROUP ROWS DST_IN DST_OUT COUNT\n"); return 2; }
    const size_t n = (size_t)std::strtoull(argv[1], nullptr, 10);
    const uint32_t stride = (uint32_t)std::strtoul(argv[2], nullptr, 10), width = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    const bool weighted = std::strtoul(argv[4], nullptr, 10) != 0;
    const size_t dst_first = (size_t)std::strtoull(argv[5], nullptr, 10), capacity = (size_t)std::strtoull(argv[6], nullptr, 10);
    if (!gs4d_rows::query_ok(stride, width, 0, 0)) return 3;
    std::vector<float> rec(weighted ? 24 * n : 0);
    std::vector<uint32_t> mg(n);
    std::vector<unsigned char> rows(n * stride), dst(capacity * stride);
    if (!slurp(argv[7], rec.data(), 4 * rec.size()) || !slurp(argv[8], mg.data(), 4 * n) || !slurp(argv[9], rows.data(), rows.size()) ||
        !slurp(argv[10], dst.data(), dst.size())) return 2;
    uint32_t count[4] = { 0, 0, 0, 0 };
    gs4d_rows::host_merge_rows(n, weighted ? rec.data() : nullptr, mg.data(), rows.data(), stride, width, 0, 0, dst.data(), dst_first, capacity, count);
    if (!spill(argv[11], dst.data(), dst.size()) || !spill(argv[12], count, sizeof(count))) return 2;
    return 0;
}
