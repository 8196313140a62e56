// decompose_record_check — the per-record text of gs4d_decompose_records (csrc/decompose_record.h, what csrc/decompose.hip evaluates on the device
// and the host library on the CPU) compiled stand-alone: tests/test_decompose_host.py builds this with `g++ -O2 -std=c++17 -ffp-contract=off` (and
// once more with -fsanitize=address,undefined,float-cast-overflow) and compares its output with gs4d_host_decompose_records (NaN words: NaN on both
// sides).  Both sides are the same text, so this checks the flags and the compilers: another compiler gives the library's bits.
//
//   decompose_record_check N FORM IN OUT [SWEEPS]
// IN: N records of 24 float32.  FORM: 0 (GS4D_PARAMS_3D) or 1 (GS4D_PARAMS_4D_VEL).  OUT: N rows of 19 float32 — pos (4; 3D: the fourth is 0),
// q (w x y z), scale (3), rgba (4), dir (3), tvar (3D: zeros).  SWEEPS: 1 .. 8 instead of the header's constant — the measurement of
// tools/decompose_sweeps.py, never what the tests run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/decompose_record.h"

constexpr int ROW = 19;

template <int FORM, int SWEEPS>
static void rows(size_t n, const float* rec, float* out) {
    for (size_t i = 0; i < n; ++i) {
        gs4d_decompose::Splat s;
        std::memset(&s, 0, sizeof s);
        gs4d_decompose::record<FORM, true, SWEEPS>(rec + 24 * i, s);
        float* o = out + ROW * i;
        std::memcpy(o, s.pos, 16); std::memcpy(o + 4, s.q, 16); std::memcpy(o + 8, s.s, 12); std::memcpy(o + 11, s.rgba, 16); std::memcpy(o + 15, s.dir, 12);
        o[18] = s.tvar;
    }
}

template <int SWEEPS>
static void forms(int form, size_t n, const float* rec, float* out) { if (form == 0) rows<0, SWEEPS>(n, rec, out); else rows<1, SWEEPS>(n, rec, out); }

int main(int argc, char** argv) {
    if (argc != 5 && argc != 6) { std::fprintf(stderr, "usage: decompose_record_check N FORM IN OUT [SWEEPS]\n"); return 2; }
    const size_t n = (size_t)std::strtoull(argv[1], nullptr, 10);
    const int form = std::atoi(argv[2]), sweeps = argc == 6 ? std::atoi(argv[5]) : gs4d_decompose::SWEEPS;
    if ((form != 0 && form != 1) || sweeps < 1 || sweeps > 8) { std::fprintf(stderr, "FORM is 0 or 1, SWEEPS 1 .. 8\n"); return 2; }
    std::vector<float> rec(n * 24), out(n * ROW);
    FILE* in = std::fopen(argv[3], "rb");
    if (!in) { std::perror(argv[3]); return 1; }
    const bool read = n == 0 || std::fread(rec.data(), 96, n, in) == n;
    std::fclose(in);
    if (!read) { std::fprintf(stderr, "%s: too short\n", argv[3]); return 1; }
    switch (sweeps) {
    case 1: forms<1>(form, n, rec.data(), out.data()); break;
    case 2: forms<2>(form, n, rec.data(), out.data()); break;
    case 3: forms<3>(form, n, rec.data(), out.data()); break;
    case 4: forms<4>(form, n, rec.data(), out.data()); break;
    case 5: forms<5>(form, n, rec.data(), out.data()); break;
    case 6: forms<6>(form, n, rec.data(), out.data()); break;
    case 7: forms<7>(form, n, rec.data(), out.data()); break;
    default: forms<8>(form, n, rec.data(), out.data()); break;
    }
    FILE* f = std::fopen(argv[4], "wb");
    if (!f) { std::perror(argv[4]); return 1; }
    const bool ok = std::fwrite(out.data(), 4, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 1;
}
