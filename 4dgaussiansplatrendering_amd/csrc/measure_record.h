// measure_record.h — what one record adds to a gs4d_measure_records measurement (include/gs4d.h), as plain C++ inline functions: the
// one text of the definition.  csrc/measure.hip evaluates it on the device, host/gs4d_host.cpp (gs4d_host_measure_records) on the CPU.  It restates
// the header's text operation by operation: float32, every product and every sum rounded on its own in the order the parentheses give (build
// without contraction), division and sqrtf correctly rounded.  The centre and the two skips are centre_query.h's own functions: the text is
// gs4d_count_centres'.  Include it after gs4d.h (GS4D_MS_*, GS4D_TIME_DEAD_ARG) and <math.h> / <cmath>.
#ifndef GS4D_MEASURE_RECORD_H
#define GS4D_MEASURE_RECORD_H

#include "centre_query.h"

namespace gs4d_measure_rec {

// what the definition reads of a record beside gs4d_centre::Fields (a: under GS4D_MS_SKIP_HIDDEN only): diag = floats 8, 13 and 18, S[a][a]
struct Fields { gs4d_centre::Fields c; float diag[3]; };

// ---- the total order of the box ends ----
// key(v) = bits ^ (sign ? 0xFFFFFFFF : 0x80000000): ascending as unsigned integers from -inf over -0 < +0 to +inf (no NaN is ever keyed).  The least
// and the greatest key of a set do not depend on the order they are found in, so neither do the bits of a box end.
GS4D_HD inline uint32_t key_of_bits(uint32_t b) { return b ^ ((b & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u); }
GS4D_HD inline uint32_t bits_of_key(uint32_t k) { return k ^ ((k & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu); }
GS4D_HD inline uint32_t bits_of(float v) { union { float f; uint32_t u; } c; c.f = v; return c.u; }
GS4D_HD inline uint32_t key_of(float v) { return key_of_bits(bits_of(v)); }
constexpr uint32_t KEY_PINF = 0xFF800000u, KEY_NINF = 0x007FFFFFu;       // the keys of +inf and -inf: the empty minimum and the empty maximum
GS4D_HD inline bool finite(float v) { return fabsf(v) < __builtin_huge_valf(); }

// ---- a measurement in the making: the first 64 bytes of gs4d_measure with keys in the place of the floats ----
// words 0..3: count, unplaced, skipped, 0 (sums); 4..6 / 7..9: keys of lo / hi; 10..12 / 13..15: keys of ext_lo / ext_hi (minima / maxima)
enum { ROW_WORDS = 16, ROW_COUNT = 0, ROW_UNPLACED = 1, ROW_SKIPPED = 2, ROW_LO = 4, ROW_HI = 7, ROW_EXT_LO = 10, ROW_EXT_HI = 13 };
GS4D_HD inline bool row_is_sum(int w) { return w < ROW_LO; }
GS4D_HD inline bool row_is_min(int w) { return (w >= ROW_LO && w < ROW_HI) || (w >= ROW_EXT_LO && w < ROW_EXT_HI); }
GS4D_HD inline uint32_t row_empty(int w) { return row_is_sum(w) ? 0u : row_is_min(w) ? KEY_PINF : KEY_NINF; }
GS4D_HD inline uint32_t row_join(int w, uint32_t a, uint32_t b) { return row_is_sum(w) ? a + b : row_is_min(w) ? (a < b ? a : b) : (a > b ? a : b); }
// what word w of gs4d_measure holds for a finished row
GS4D_HD inline uint32_t row_word(int w, uint32_t v) { return row_is_sum(w) ? v : bits_of_key(v); }

// ---- one selected record ----
enum { SKIPPED = 0, UNPLACED = 1, MEASURED = 2 };
// the centre at time t, the skips, "placed".  m is the centre when the answer is MEASURED.
GS4D_HD inline int place(float t, uint32_t flags, const gs4d_centre::Fields& r, float m[3]) {
    const float dt = gs4d_centre::centre_at(t, r, m);
    if ((flags & (uint32_t)GS4D_MS_SKIP_HIDDEN) && gs4d_centre::hidden(r)) return SKIPPED;
    if ((flags & (uint32_t)GS4D_MS_SKIP_DEAD) && gs4d_centre::dead_at(dt, r)) return SKIPPED;
    return finite(m[0]) && finite(m[1]) && finite(m[2]) ? MEASURED : UNPLACED;
}
// the reach along axis a: three standard deviations of the spatial variance conditioned on the time
GS4D_HD inline float reach(const Fields& r, int a) {
    const float var = r.diag[a] - ((r.c.sig3[a] * r.c.sig3[a]) * (1.0f / r.c.s44));
    return var > 0.0f ? 3.0f * sqrtf(var) : 0.0f;
}
// a selected record into a row
GS4D_HD inline void add_record(float t, uint32_t flags, const Fields& r, uint32_t (&row)[ROW_WORDS]) {
    float m[3];
    const int what = place(t, flags, r.c, m);
    if (what == SKIPPED) { row[ROW_SKIPPED] += 1u; return; }
    if (what == UNPLACED) { row[ROW_UNPLACED] += 1u; return; }
    row[ROW_COUNT] += 1u;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const uint32_t k = key_of(m[a]);
        row[ROW_LO + a] = row[ROW_LO + a] < k ? row[ROW_LO + a] : k;
        row[ROW_HI + a] = row[ROW_HI + a] > k ? row[ROW_HI + a] : k;
        const float rr = reach(r, a);
        const float e0 = m[a] - rr, e1 = m[a] + rr;
        if (finite(e0)) { const uint32_t k0 = key_of(e0); row[ROW_EXT_LO + a] = row[ROW_EXT_LO + a] < k0 ? row[ROW_EXT_LO + a] : k0; }
        if (finite(e1)) { const uint32_t k1 = key_of(e1); row[ROW_EXT_HI + a] = row[ROW_EXT_HI + a] > k1 ? row[ROW_EXT_HI + a] : k1; }
    }
}
// the cell of a measured centre's coordinate in the finished box, 0 .. 2^20 (gs4d_spatial_order's form: a NaN from e == 0 or an overflowed e gives 0)
GS4D_HD inline uint32_t cell(float m, float lo, float hi) {
    const float d = m - lo, e = hi - lo;
    const float g = (d / e) * 1048576.0f;
    return g >= 0.0f ? (uint32_t)(g < 1048576.0f ? g : 1048576.0f) : 0u;
}

} // namespace gs4d_measure_rec
#endif
