// pose_record_check — the per-record text of gs4d_pose_records (csrc/pose_record.h, what csrc/pose.hip evaluates on the device and the host library
// on the CPU) compiled stand-alone: tests/test_pose_host.py builds this with `g++ -O2 -std=c++17 -ffp-contract=off` (and once more with
// -fsanitize=address,undefined) and compares its output with gs4d_host_pose_records (NaN words: NaN on both sides).  Both sides are the same text, so
// this checks the flags and the compilers: another compiler gives the library's bits.  The buffers are allocated at exactly the sizes the call
// demands, so the instrumented build also shows that of bind only rows < n and of xf only rows < m are read.
//
//   pose_record_check N M FORM STRIDE IN XF BIND OUT
// IN: N records of 24 float32.  XF: M rows of 20 float32.  BIND: N rows of STRIDE bytes.  FORM: 0 (index) or 1 (blend4).  OUT: N records.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/pose_record.h"

struct Row { float v[20]; };                                                      // gs4d_affine4
static_assert(sizeof(Row) == 80, "the structure of include/gs4d.h");

static bool slurp(const char* path, void* to, size_t bytes) {
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::perror(path); return false; }
    const bool ok = bytes == 0 || std::fread(to, 1, bytes, in) == bytes;
    std::fclose(in);
    if (!ok) std::fprintf(stderr, "%s: too short\n", path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 9) { std::fprintf(stderr, "usage: pose_record_check N M FORM STRIDE IN XF BIND OUT\n"); return 2; }
    const size_t n = (size_t)std::strtoull(argv[1], nullptr, 10), m = (size_t)std::strtoull(argv[2], nullptr, 10);
    const unsigned form = (unsigned)std::strtoul(argv[3], nullptr, 10);
    const size_t stride = (size_t)std::strtoull(argv[4], nullptr, 10);
    if (form > 1u || stride < (form ? 32u : 4u) || stride % (form ? 16u : 4u) != 0 || m > 0xFFFFFFFFull) { std::fprintf(stderr, "a form or a stride the call refuses\n"); return 2; }
    std::vector<float> rec(n * 24), out(n * 24);
    std::vector<Row> xf(m);
    std::vector<unsigned char> bind(n * stride);
    if (!slurp(argv[5], rec.data(), n * 96) || !slurp(argv[6], xf.data(), m * 80) || !slurp(argv[7], bind.data(), n * stride)) return 1;
    const Row* const table = xf.data();
    const auto rows = [table](unsigned int j, float r[20]) { std::memcpy(r, table[j].v, 80); };
    for (size_t i = 0; i < n; ++i) {
        const unsigned char* const row = bind.data() + i * stride;
        if (form == 0u) {
            uint32_t j;
            std::memcpy(&j, row, 4);
            gs4d_pose::index(rows, (unsigned int)m, j, &rec[24 * i], &out[24 * i]);
        } else {
            unsigned int j[4];
            float w[4];
            std::memcpy(j, row, 16);
            std::memcpy(w, row + 16, 16);
            gs4d_pose::blend(rows, (unsigned int)m, j, w, &rec[24 * i], &out[24 * i]);
        }
    }
    FILE* f = std::fopen(argv[8], "wb");
    if (!f) { std::perror(argv[8]); return 1; }
    const bool ok = std::fwrite(out.data(), 4, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 1;
}
