// transform_selected_check — the per-record text of gs4d_transform_selected and the centre of a measurement (csrc/transform_record.h, what
// csrc/transform_selected.hip evaluates on the device and the host library on the CPU) compiled stand-alone: tests/test_xfsel_host.py builds this
// with `g++ -O2 -std=c++17 -ffp-contract=off` (and once more with -fsanitize=address,undefined) and compares its output with
// gs4d_host_transform_selected and gs4d_host_measure_centre (NaN words: NaN on both sides).  Both sides are the same text, so this checks the flags
// and the compilers: another compiler gives the library's bits.
//
//   transform_selected_check N M IN SEL XF MEASURE OUT
// IN: N records of 24 float32.  SEL: N bytes, non-zero: the record is selected.  XF: M rows of 96 bytes (gs4d_selection_xf: l[16], o[4], pivot[3],
// flags).  MEASURE: the 96 bytes of a gs4d_measure.  OUT: the centre of MEASURE (3 float32), then M * N records, row after row: the selected ones
// under the row, the others as they were.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/transform_record.h"

struct Row { float l[16], o[4], pivot[3]; uint32_t flags; };                      // gs4d_selection_xf
struct Measure { uint32_t count, unplaced, skipped, reserved0; float lo[3], hi[3], ext_lo[3], ext_hi[3]; unsigned long long cell_sum[3], reserved1; };      // gs4d_measure
static_assert(sizeof(Row) == 96 && sizeof(Measure) == 96, "the structures of include/gs4d.h");

static bool slurp(const char* path, void* to, size_t bytes) {
    FILE* in = std::fopen(path, "rb");
    if (!in) { std::perror(path); return false; }
    const bool ok = bytes == 0 || std::fread(to, 1, bytes, in) == bytes;
    std::fclose(in);
    if (!ok) std::fprintf(stderr, "%s: too short\n", path);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: transform_selected_check N M IN SEL XF MEASURE OUT\n"); return 2; }
    const size_t n = (size_t)std::strtoull(argv[1], nullptr, 10), m = (size_t)std::strtoull(argv[2], nullptr, 10);
    std::vector<float> rec(n * 24), out(3 + m * n * 24);
    std::vector<unsigned char> sel(n);
    std::vector<Row> rows(m);
    Measure ms;
    if (!slurp(argv[3], rec.data(), n * 96) || !slurp(argv[4], sel.data(), n) || !slurp(argv[5], rows.data(), m * 96) || !slurp(argv[6], &ms, 96)) return 1;
    float centre[3];
    gs4d_transform::measure_centre(ms.count, ms.lo, ms.hi, ms.cell_sum, centre);
    std::memcpy(out.data(), centre, sizeof centre);
    for (size_t j = 0; j < m; ++j) {
        const Row& x = rows[j];
        const float* const c = x.flags == 2u ? centre : x.pivot;                  // GS4D_XS_PIVOT_MEASURE
        for (size_t i = 0; i < n; ++i) {
            float* const o = &out[3 + 24 * (j * n + i)];
            if (sel[i]) gs4d_transform::record_about(x.l, x.o, x.flags != 0u, c, &rec[24 * i], o);
            else std::memcpy(o, &rec[24 * i], 96);
        }
    }
    FILE* f = std::fopen(argv[7], "wb");
    if (!f) { std::perror(argv[7]); return 1; }
    const bool ok = std::fwrite(out.data(), 4, out.size(), f) == out.size();
    return (std::fclose(f) == 0 && ok) ? 0 : 1;
}
