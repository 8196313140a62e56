// Stand-alone check of csrc/operands.h: the buffer-argument check of the record-set calls, over a table of buffers of its own.
// Prints one line per group of cases and exits 0 when every case holds.  tests/test_operands_host.py builds it plainly and with
// AddressSanitizer + UndefinedBehaviorSanitizer (an executable of its own) and runs it.
#include "../4dgaussiansplatrendering_amd/csrc/operands.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

using namespace gs4d;

static std::map<uint32_t, BufferFacts> g_bufs;      // name -> {live, bytes}; a name that is not here is unknown
static BufferFacts lookup(uint32_t name) { auto it = g_bufs.find(name); return it == g_bufs.end() ? BufferFacts{ false, 0 } : it->second; }
static OperandVerdict run(const std::vector<Operand>& ops) { return check_operand_list(ops.data(), (int)ops.size(), lookup); }

static int g_failed = 0, g_cases = 0;
static void expect(const char* what, const std::vector<Operand>& ops, OperandFault fault, int at, int other = -1) {
    const OperandVerdict v = run(ops);
    ++g_cases;
    bool ok = v.fault == fault && v.at == at && v.other == other;
    if (ok && fault != OperandFault::None) {      // the message has the prefix and names the operand made bad
        const std::string m = operand_message("fn", ops.data(), v), head = std::string("fn: ") + ops[at].arg;
        ok = m.compare(0, head.size(), head) == 0 && m.size() > head.size();
        if (fault == OperandFault::Same) ok = ok && m.find(ops[other].arg) != std::string::npos;
    }
    if (!ok) { ++g_failed; printf("FAILED %s: fault %d at %d (other %d), expected %d at %d (other %d)\n", what, (int)v.fault, v.at, v.other, (int)fault, at, other); }
}

int main() {
    // buffers 1..4 hold 300 rows of 96, 16, 1024 and 4 bytes; 5 is destroyed; 6 is empty; 7 holds 96 bytes; 9999 is unknown
    g_bufs = { { 1, { true, 300 * 96 } }, { 2, { true, 300 * 16 } }, { 3, { true, 300 * 1024 } }, { 4, { true, 300 * 4 } }, { 5, { false, 4096 } }, { 6, { true, 0 } }, { 7, { true, 96 } } };
    const unsigned R = OP_READ, W = OP_WRITE;

    // names
    expect("good call", { { "a", 1, false, 96, 300, R }, { "b", 2, false, 16, 300, W } }, OperandFault::None, -1);
    expect("required 0", { { "a", 1, false, 96, 300, R }, { "b", 0, false, 16, 300, W } }, OperandFault::Missing, 1);
    expect("required 0 first", { { "a", 0, false, 96, 300, R }, { "b", 2, false, 16, 300, W } }, OperandFault::Missing, 0);
    expect("dead", { { "a", 1, false, 96, 300, R }, { "b", 5, false, 16, 1, W } }, OperandFault::NotLive, 1);
    expect("dead optional", { { "a", 1, false, 96, 300, R }, { "b", 5, true, 16, 1, W } }, OperandFault::NotLive, 1);
    expect("unknown", { { "a", 9999, false, 96, 300, R }, { "b", 2, false, 16, 300, W } }, OperandFault::NotLive, 0);
    expect("unknown optional", { { "a", 1, false, 96, 300, R }, { "b", 9999, true, 16, 300, W } }, OperandFault::NotLive, 1);
    expect("optional 0", { { "a", 1, false, 96, 300, R }, { "b", 0, true, 16, 300, W } }, OperandFault::None, -1);
    expect("two optional 0", { { "a", 0, true, 96, 300, R }, { "b", 1, false, 96, 300, R }, { "c", 0, true, 16, 300, W } }, OperandFault::None, -1);
    expect("optional 0 with a row of 0 bytes", { { "a", 0, true, 0, 300, R }, { "b", 1, false, 96, 300, R } }, OperandFault::None, -1);
    printf("names: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // each pair of equal names among four operands; the later one is reported, with the earlier one as `other`
    for (int i = 0; i < 4; ++i) for (int j = i + 1; j < 4; ++j) {
        std::vector<Operand> ops = { { "a", 1, false, 1, 1, R }, { "b", 2, true, 1, 1, R }, { "c", 3, false, 1, 1, W }, { "d", 4, true, 1, 1, W } };
        ops[j].name = ops[i].name;
        expect("equal names", ops, OperandFault::Same, j, i);
    }
    // a name fault is decided before any size fault
    expect("same before short", { { "a", 1, false, 96, 301, R }, { "b", 1, false, 96, 300, W } }, OperandFault::Same, 1, 0);
    printf("pairs: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // an exact fit and one byte short, rows of 16, 96 and 1024 bytes
    const size_t widths[3] = { 16, 96, 1024 };
    for (size_t w : widths) {
        g_bufs[10] = { true, 300 * w };
        expect("exact fit", { { "a", 1, false, 96, 300, R }, { "x", 10, false, w, 300, W } }, OperandFault::None, -1);
        g_bufs[10] = { true, 300 * w - 1 };
        expect("one byte short", { { "a", 1, false, 96, 300, R }, { "x", 10, false, w, 300, W } }, OperandFault::Short, 1);
        expect("one byte short, first", { { "x", 10, false, w, 300, W }, { "a", 1, false, 96, 300, R } }, OperandFault::Short, 0);
        g_bufs[10] = { true, 300 * w + (w - 1) };
        expect("a partial row counts for nothing", { { "x", 10, false, w, 301, W } }, OperandFault::Short, 0);
    }
    // rows = 2^64 - 1 of 1024 bytes: refused, and no product is formed that could wrap (UBSan watches the signed ones, the result the unsigned)
    g_bufs[10] = { true, ~(size_t)0 };
    expect("2^64 - 1 rows", { { "x", 10, false, 1024, ~0ull, W } }, OperandFault::Short, 0);
    expect("2^54 rows need 2^64 bytes",{ { "x", 10, false, 1024, 1ull << 54, W } }, OperandFault::Short, 0);      // 2^64 - 1 bytes hold 2^54 - 1 whole rows
    expect("2^54 - 1 rows fit", { { "x", 10, false, 1024, (1ull << 54) - 1, W } }, OperandFault::None, -1);
    expect("a sum above 2^32 stays 64-bit", { { "a", 1, false, 96, 0xFFFFFFFFull + 300ull, W } }, OperandFault::Short, 0);
    printf("sizes: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // byte-count operands (row == 1) of 8, 16 and 96 bytes
    const size_t counts[3] = { 8, 16, 96 };
    for (size_t b : counts) {
        g_bufs[11] = { true, b };
        expect("byte count fits", { { "out", 11, false, 1, b, W } }, OperandFault::None, -1);
        g_bufs[11] = { true, b - 1 };
        expect("byte count one short", { { "a", 1, false, 96, 300, R }, { "out", 11, false, 1, b, W } }, OperandFault::Short, 1);
        const std::string m = operand_message("fn", std::vector<Operand>{ { "out", 11, false, 1, b, W } }.data(), { OperandFault::Short, 0, -1 });
        ++g_cases;
        if (m != "fn: out holds fewer than " + std::to_string(b) + " bytes") { ++g_failed; printf("FAILED message: %s\n", m.c_str()); }
    }
    // zero rows against an empty buffer, and an empty buffer against one row
    expect("zero rows, empty buffer", { { "a", 6, false, 96, 0, R }, { "b", 1, false, 96, 0, W } }, OperandFault::None, -1);
    expect("one row, empty buffer", { { "a", 6, false, 96, 1, R } }, OperandFault::Short, 0);
    expect("one row of 96 in 96 bytes", { { "a", 7, false, 96, 1, R } }, OperandFault::None, -1);
    printf("byte counts and empty buffers: ok so far %d of %d\n", g_cases - g_failed, g_cases);

    // the operand reported is the one made bad: an eight-operand list (gs4d_build_records' length), one fault at each place in turn
    for (int bad = 0; bad < 8; ++bad) for (int kind = 0; kind < 4; ++kind) {
        std::vector<Operand> ops;
        const char* const args[8] = { "pos", "rot", "rot_r", "scale", "rgba", "dir", "tvar", "dst" };
        for (uint32_t k = 0; k < 8; ++k) { g_bufs[20 + k] = { true, 300 * 16 }; ops.push_back({ args[k], 20 + k, false, 16, 300, k == 7 ? W : R }); }
        if (kind == 0) ops[bad].name = 0;
        if (kind == 1) ops[bad].name = 5;
        if (kind == 2) ops[bad].name = 9999;
        if (kind == 3) g_bufs[20 + bad].bytes -= 1;
        expect("the one made bad", ops, kind == 0 ? OperandFault::Missing : kind == 3 ? OperandFault::Short : OperandFault::NotLive, bad);
    }
    printf("%d cases, %d failed\n", g_cases, g_failed);
    return g_failed ? 1 : 0;
}
