// build_record_check — the per-record text of gs4d_build_records (csrc/build_record.h, what csrc/build.hip evaluates on the device and the host
// library on the CPU) compiled stand-alone: tests/test_build_host.py builds this with `g++ -O2 -std=c++17 -ffp-contract=off` and compares its output
// bit for bit with the host builders.  Both sides are the same text, so this checks the flags and the compilers: another compiler gives the library's bits.
//
//   build_record_check FORM N IN OUT
// FORM: 0 / 1 / 2 = GS4D_PARAMS_3D / _4D_VEL / _4D_2Q.  IN: the form's parameter arrays one after another, in the order of gs4d_splat_params (pos, rot,
// rot_r, scale, rgba, dir, tvar; only those the form uses), each N tightly packed float32 rows.  OUT: N records of 24 floats.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/build_record.h"

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage: build_record_check FORM N IN OUT\n"); return 2; }
    const int form = std::atoi(argv[1]);
    const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
    if (form < 0 || form > 2) { std::fprintf(stderr, "unknown form\n"); return 2; }
    //                          pos rot rot_r scale rgba dir tvar
    static const size_t width[3][7] = { { 3, 4, 0, 3, 4, 0, 0 }, { 4, 4, 0, 3, 4, 3, 1 }, { 4, 4, 4, 4, 4, 0, 0 } };
    std::vector<float> a[7];
    FILE* in = std::fopen(argv[3], "rb");
    if (!in) { std::perror(argv[3]); return 1; }
    for (int k = 0; k < 7; ++k) {
        a[k].resize(n * width[form][k]);
        if (!a[k].empty() && std::fread(a[k].data(), 4, a[k].size(), in) != a[k].size()) { std::fprintf(stderr, "%s: too short\n", argv[3]); return 1; }
    }
    std::fclose(in);
    std::vector<float> rec(n * 24);
    for (size_t i = 0; i < n; ++i) {
        float* o = rec.data() + 24 * i;
        if (form == 0) gs4d_build::record_3d(&a[0][3 * i], &a[1][4 * i], &a[3][3 * i], &a[4][4 * i], o);
        else if (form == 1) gs4d_build::record_4d_vel(&a[0][4 * i], &a[1][4 * i], &a[3][3 * i], &a[5][3 * i], a[6][i], &a[4][4 * i], o);
        else gs4d_build::record_4d_2q(&a[0][4 * i], &a[1][4 * i], &a[2][4 * i], &a[3][4 * i], &a[4][4 * i], o);
    }
    FILE* out = std::fopen(argv[4], "wb");
    if (!out) { std::perror(argv[4]); return 1; }
    const bool ok = rec.empty() || std::fwrite(rec.data(), 4, rec.size(), out) == rec.size();
    return (std::fclose(out) == 0 && ok) ? 0 : 1;
}
