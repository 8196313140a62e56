// sh_rotate_check — the per-row text of gs4d_rotate_sh (csrc/sh_rotate_record.h, what csrc/sh_rotate.hip evaluates on the device and the host library
// on the CPU) and the call's context-free checks (csrc/sh_rotate_operands.h) compiled stand-alone: tests/test_sh_rotate_host.py builds this with
// `g++ -O2 -std=c++17 -ffp-contract=off` (and once more with -fsanitize=address,undefined) and compares its output with gs4d_host_rotate_sh (NaN
// words: NaN on both sides).  Both sides are the same text, so this checks the flags and the compilers: another compiler gives the library's bits.
// The buffers are allocated at exactly the sizes the call demands, so the instrumented build also shows that of bind only rows < n, of xf only rows
// < m and of a row only its stride are touched.
//
//   sh_rotate_check rows N STRIDE DEGREE M FORM BIND_STRIDE IN XF BIND OUT
//       IN: N rows of STRIDE bytes.  XF: M rows of 20 float32.  BIND: N rows of BIND_STRIDE bytes (FORM 0, 1; not opened for FORM 2).  OUT: the rows
//       the call writes (M * N for FORM 2, else N).  Arguments the call refuses: exit status 3, nothing written.
//   sh_rotate_check matrices XF OUT
//       XF: 20 float32.  OUT: 85 float32 — d[84] (zeros where the map does not rotate), then 1.0 or 0.0.
//   sh_rotate_check args
//       the scalar rules and the operand list over a table of buffers of its own; exit status 0 iff every verdict is the expected one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/sh_rotate_operands.h"
#include "../4dgaussiansplatrendering_amd/csrc/sh_rotate_record.h"

struct Map { float v[20]; };                                                      // gs4d_affine4
static_assert(sizeof(Map) == 80, "the structure of include/gs4d.h");

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
    return std::fclose(f) == 0 && ok;
}

template <int DEGREE>
static void rotate_rows(size_t n, const unsigned char* rows, size_t stride, const Map* xf, size_t m, const unsigned char* bind, unsigned form, size_t bind_stride,
                        unsigned char* out) {
    constexpr size_t used = 12u * (size_t)gs4d_shrot::coeffs(DEGREE);
    const auto table = [xf](unsigned int j, float r[20]) { std::memcpy(r, xf[j].v, 80); };
    const size_t instances = form == gs4d::SHROT_EACH ? m : 1;
    for (size_t inst = 0; inst < instances; ++inst)
        for (size_t i = 0; i < n; ++i) {
            const unsigned char* const row = rows + i * stride;
            unsigned char* const to = out + (inst * n + i) * stride;
            std::memcpy(to, row, stride);
            if (DEGREE == 0) continue;
            float a[20];
            bool mapped;
            if (form == gs4d::SHROT_EACH) {
                table((unsigned int)inst, a);
                mapped = true;
            } else if (form == gs4d::SHROT_INDEX) {
                uint32_t j;
                std::memcpy(&j, bind + i * bind_stride, 4);
                mapped = gs4d_shrot::index_map(table, (unsigned int)m, j, a);
            } else {
                unsigned int j[4];
                float w[4];
                std::memcpy(j, bind + i * bind_stride, 16);
                std::memcpy(w, bind + i * bind_stride + 16, 16);
                mapped = gs4d_pose::blend4(table, (unsigned int)m, j, w, a);
            }
            if (!mapped) continue;
            float c[used / 4];
            std::memcpy(c, row, used);
            if (gs4d_shrot::coefficients<DEGREE>(a, c)) std::memcpy(to + 12, c + 3, used - 12);
        }
}

static int run_rows(char** argv) {
    const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10), stride = (size_t)std::strtoull(argv[3], nullptr, 10);
    const int degree = (int)std::strtol(argv[4], nullptr, 10);
    const size_t m = (size_t)std::strtoull(argv[5], nullptr, 10);
    const unsigned form = (unsigned)std::strtoul(argv[6], nullptr, 10);
    const size_t bind_stride = (size_t)std::strtoull(argv[7], nullptr, 10);
    const bool each = form == gs4d::SHROT_EACH;
    if (gs4d::rotate_sh_fault(n, stride, degree, m, !each, form, bind_stride, 0)) return 3;
    std::vector<unsigned char> rows(n * stride), bind(each ? 0 : n * bind_stride), out(gs4d::rotate_sh_rows(n, m, form) * stride);
    std::vector<Map> xf(m);
    if (!slurp(argv[8], rows.data(), rows.size()) || !slurp(argv[9], xf.data(), m * 80) || (!each && !slurp(argv[10], bind.data(), bind.size()))) return 1;
    (degree == 0 ? &rotate_rows<0> : degree == 1 ? &rotate_rows<1> : degree == 2 ? &rotate_rows<2> : &rotate_rows<3>)(n, rows.data(), stride, xf.data(), m, bind.data(), form,
                                                                                                                   bind_stride, out.data());
    return spill(argv[11], out.data(), out.size()) ? 0 : 1;
}

static int run_matrices(char** argv) {
    Map map;
    if (!slurp(argv[2], map.v, 80)) return 1;
    std::vector<float> l(map.v, map.v + 16), d(85, 0.0f);                          // (l at its exact size: the frame reads no offset)
    d[84] = gs4d_shrot::rotation<3>(l.data(), d.data()) ? 1.0f : 0.0f;
    return spill(argv[3], d.data(), 85 * 4) ? 0 : 1;
}

// ---- the checks -------------------------------------------------------------------------------------------------------------------------------------
static int failures = 0;
static void expect(bool ok, const char* what) { if (!ok) { std::fprintf(stderr, "args: %s\n", what); ++failures; } }

static int run_args() {
    using namespace gs4d;
    const uint64_t big = 1ull << 32;
    // the scalar rules: (n, stride, degree, m, bind given, form, bind_stride, dst_first)
    expect(!rotate_sh_fault(300, 192, 3, 3, false, SHROT_EACH, 0, 5), "a valid EACH call is refused");
    expect(!rotate_sh_fault(300, 208, 3, 3, true, SHROT_INDEX, 4, 5), "a valid INDEX call is refused");
    expect(!rotate_sh_fault(300, 1024, 2, 0, true, SHROT_BLEND4, 48, 0), "a valid BLEND4 call with m == 0 is refused");
    expect(!rotate_sh_fault(0, 16, 0, 0, false, SHROT_EACH, 12345, 0xFFFFFFFFull), "n == 0, m == 0 with EACH is refused");
    expect(!rotate_sh_fault(0xFFFFFFFFull, 16, 0, 1, false, SHROT_EACH, 0, 0), "2^32 - 1 rows are refused");
    expect(rotate_sh_fault(big, 192, 3, 1, false, SHROT_EACH, 0, 0), "n above 2^32 - 1");
    expect(rotate_sh_fault(1, 192, 3, big, false, SHROT_EACH, 0, 0), "m above 2^32 - 1");
    expect(rotate_sh_fault(1, 192, 3, 1, false, SHROT_EACH, 0, big), "dst_first above 2^32 - 1");
    expect(rotate_sh_fault(1u << 16, 192, 3, 1u << 16, false, SHROT_EACH, 0, 0), "m * n above 2^32 - 1");
    expect(rotate_sh_fault(1u << 16, 192, 3, (1u << 16) - 1, false, SHROT_EACH, 0, 1u << 16), "dst_first + m * n above 2^32 - 1");
    expect(!rotate_sh_fault(1u << 16, 192, 3, 1u << 16, true, SHROT_INDEX, 4, 0), "m * n does not matter with a bind table");
    expect(rotate_sh_fault(300, 192, 3, 3, true, SHROT_INDEX, 4, big - 300), "dst_first + n above 2^32 - 1");
    expect(rotate_sh_fault(1, 192, -1, 1, false, SHROT_EACH, 0, 0) && rotate_sh_fault(1, 1024, 4, 1, false, SHROT_EACH, 0, 0), "a degree outside 0 .. 3");
    for (uint64_t stride : { 0ull, 8ull, 24ull, 200ull, 1040ull, 2048ull }) expect(rotate_sh_fault(1, stride, 0, 1, false, SHROT_EACH, 0, 0), "a stride that breaks the rule");
    expect(rotate_sh_fault(1, 32, 1, 1, false, SHROT_EACH, 0, 0) && rotate_sh_fault(1, 96, 2, 1, false, SHROT_EACH, 0, 0) && rotate_sh_fault(1, 176, 3, 1, false, SHROT_EACH, 0, 0),
           "a stride below 12 (degree + 1)^2");
    expect(!rotate_sh_fault(1, 48, 1, 1, false, SHROT_EACH, 0, 0) && !rotate_sh_fault(1, 112, 2, 1, false, SHROT_EACH, 0, 0), "the minimal strides are refused");
    expect(rotate_sh_fault(1, 192, 3, 1, false, 3u, 0, 0) && rotate_sh_fault(1, 192, 3, 1, true, 0xFFFFFFFFu, 4, 0), "an unknown form");
    expect(rotate_sh_fault(1, 192, 3, 1, true, SHROT_EACH, 4, 0), "bind with EACH");
    expect(rotate_sh_fault(1, 192, 3, 1, false, SHROT_INDEX, 4, 0) && rotate_sh_fault(1, 192, 3, 1, false, SHROT_BLEND4, 32, 0), "no bind with a bind form");
    for (uint64_t bs : { 0ull, 2ull, 6ull }) expect(rotate_sh_fault(1, 192, 3, 1, true, SHROT_INDEX, bs, 0), "an INDEX bind_stride that breaks the rule");
    for (uint64_t bs : { 0ull, 16ull, 40ull }) expect(rotate_sh_fault(1, 192, 3, 1, true, SHROT_BLEND4, bs, 0), "a BLEND4 bind_stride that breaks the rule");
    expect(!rotate_sh_fault(1, 192, 3, 1, true, SHROT_INDEX, 12, 0) && !rotate_sh_fault(1, 192, 3, 1, true, SHROT_BLEND4, 48, 0), "the wider bind strides are refused");

    // the operand list over buffers of its own: name -> bytes (0: not live)
    const size_t n = 300, m = 3, stride = 208, first = 5;
    const auto facts = [&](uint32_t name) {
        switch (name) {
        case 1: return BufferFacts{ true, n * stride };                      // src
        case 2: return BufferFacts{ true, m * 80 };                          // xf
        case 3: return BufferFacts{ true, n * 32 };                          // bind (BLEND4, stride 32)
        case 4: return BufferFacts{ true, (first + n) * stride };            // dst of a bind form
        case 5: return BufferFacts{ true, (first + m * n) * stride };        // dst of EACH
        case 6: return BufferFacts{ true, n * stride - 1 };                  // a short src
        case 7: return BufferFacts{ true, m * 80 - 1 };                      // a short xf
        case 8: return BufferFacts{ true, n * 32 - 1 };                      // a short bind
        case 9: return BufferFacts{ true, (first + n) * stride - 1 };        // a short dst
        default: return BufferFacts{ false, 0 };
        }
    };
    const auto verdict = [&](uint32_t src, uint32_t xf, uint32_t bind, uint32_t form, uint32_t dst, uint64_t mm) {
        Operand op[ROTATE_SH_OPERANDS];
        rotate_sh_operands(op, src, n, stride, xf, mm, bind, form, 32, dst, first);
        expect(op[0].roles == OP_READ && op[1].roles == OP_READ && op[2].roles == OP_READ && op[3].roles == OP_WRITE, "src, xf and bind are read, dst is written");
        return check_operand_list(op, ROTATE_SH_OPERANDS, facts);
    };
    expect(verdict(1, 2, 3, SHROT_BLEND4, 4, m).fault == OperandFault::None, "a valid BLEND4 list");
    expect(verdict(1, 2, 0, SHROT_EACH, 5, m).fault == OperandFault::None, "a valid EACH list (no bind)");
    expect(verdict(1, 2, 0, SHROT_EACH, 4, m).fault == OperandFault::Short, "EACH needs dst_first + m * n rows");
    expect(verdict(1, 2, 3, SHROT_BLEND4, 4, 0).fault == OperandFault::None, "m == 0 with a bind table");
    expect(verdict(1, 2, 3, SHROT_BLEND4, 4, m + 1).fault == OperandFault::Short, "xf too small for m");
    expect(verdict(6, 2, 3, SHROT_BLEND4, 4, m).fault == OperandFault::Short && verdict(6, 2, 3, SHROT_BLEND4, 4, m).at == 0, "a short src");
    expect(verdict(1, 7, 3, SHROT_BLEND4, 4, m).fault == OperandFault::Short && verdict(1, 7, 3, SHROT_BLEND4, 4, m).at == 1, "a short xf");
    expect(verdict(1, 2, 8, SHROT_BLEND4, 4, m).fault == OperandFault::Short && verdict(1, 2, 8, SHROT_BLEND4, 4, m).at == 2, "a short bind");
    expect(verdict(1, 2, 3, SHROT_BLEND4, 9, m).fault == OperandFault::Short && verdict(1, 2, 3, SHROT_BLEND4, 9, m).at == 3, "a short dst");
    expect(verdict(0, 2, 3, SHROT_BLEND4, 4, m).fault == OperandFault::Missing && verdict(1, 0, 3, SHROT_BLEND4, 4, m).fault == OperandFault::Missing &&
           verdict(1, 2, 0, SHROT_BLEND4, 4, m).fault == OperandFault::Missing && verdict(1, 2, 3, SHROT_BLEND4, 0, m).fault == OperandFault::Missing, "a buffer that is 0");
    expect(verdict(99, 2, 3, SHROT_BLEND4, 4, m).fault == OperandFault::NotLive && verdict(1, 2, 3, SHROT_BLEND4, 99, m).fault == OperandFault::NotLive, "a name that is not live");
    expect(verdict(1, 1, 3, SHROT_BLEND4, 4, m).fault == OperandFault::Same && verdict(1, 2, 1, SHROT_BLEND4, 4, m).fault == OperandFault::Same &&
           verdict(1, 2, 3, SHROT_BLEND4, 1, m).fault == OperandFault::Same && verdict(1, 2, 2, SHROT_BLEND4, 4, m).fault == OperandFault::Same &&
           verdict(1, 2, 3, SHROT_BLEND4, 2, m).fault == OperandFault::Same && verdict(1, 2, 3, SHROT_BLEND4, 3, m).fault == OperandFault::Same, "two buffers that are the same");
    const OperandVerdict v = verdict(1, 2, 3, SHROT_BLEND4, 9, m);
    Operand op[ROTATE_SH_OPERANDS];
    rotate_sh_operands(op, 1, n, stride, 2, m, 3, SHROT_BLEND4, 32, 9, first);
    expect(operand_message("rotate_sh", op, v).find("rotate_sh: dst holds fewer than 305 rows of 208 bytes") == 0, "the message of a short dst");
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 12 && !std::strcmp(argv[1], "rows")) return run_rows(argv);
    if (argc == 4 && !std::strcmp(argv[1], "matrices")) return run_matrices(argv);
    if (argc == 2 && !std::strcmp(argv[1], "args")) return run_args();
    std::fprintf(stderr, "usage: sh_rotate_check rows N STRIDE DEGREE M FORM BIND_STRIDE IN XF BIND OUT | matrices XF OUT | args\n");
    return 2;
}
