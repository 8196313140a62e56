// transform_record_check — the per-record text of gs4d_transform_records (csrc/transform_record.h, what csrc/transform.hip evaluates on the device
// and the host library on the CPU) compiled stand-alone: tests/test_transform_host.py builds this with `g++ -O2 -std=c++17 -ffp-contract=off` and
// compares its output with gs4d_host_transform_records (NaN words: NaN on both sides).  Both sides are the same text, so this checks the flags and the
// compilers: another compiler gives the library's bits.
//
//   transform_record_check N M IN XF OUT
// IN: N records of 24 float32.  XF: M rows of 20 float32 (l[16], o[4]).  OUT: M * N records, instance after instance.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/transform_record.h"

static bool slurp(const char* path, std::vector<float>& a) {
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::perror(path); return false; }
    const bool ok = a.empty() || std::fread(a.data(), 4, a.size(), in) == a.size();
    std::fclose(in);
    if (!ok) std::fprintf(stderr, "%s: too short\n", path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 6) { std::fprintf(stderr, "usage: transform_record_check N M IN XF OUT\n"); return 2; }
    const size_t n = (size_t)std::strtoull(argv[1], nullptr, 10), m = (size_t)std::strtoull(argv[2], nullptr, 10);
    std::vector<float> rec(n * 24), xf(m * 20), out(m * n * 24);
    if (!slurp(argv[3], rec) || !slurp(argv[4], xf)) return 1;
    for (size_t j = 0; j < m; ++j)
        for (size_t i = 0; i < n; ++i) gs4d_transform::record(&xf[20 * j], &xf[20 * j + 16], &rec[24 * i], &out[24 * (j * n + i)]);
    FILE* f = std::fopen(argv[5], "wb");
    if (!f) { std::perror(argv[5]); return 1; }
    const bool ok = out.empty() || std::fwrite(out.data(), 4, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 1;
}
