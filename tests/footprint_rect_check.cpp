// footprint_rect_check.cpp — containment check of the tightened pixel rectangle (csrc/footprint_rect.h), a stand-alone program
// (tests/test_cull_host.py builds and runs it, plainly and with AddressSanitizer + UndefinedBehaviorSanitizer).  Build with -ffp-contract=off.
//
// For every record of the sets below it forms the window-space quad as emit() of csrc/preprocess.hip does (same expressions, same order), the
// OLD rectangle (the quad's box) and the NEW one (gs4d_footprint::tighten), and evaluates the compositor's own predicate, written as
// composite_chunk and blend_fragment of csrc/composite_common.h write it, on EVERY pixel of the old rectangle:
//     dx = fx - cx, dy = fy - cy;  u = fma(a0x, dx, a0y * dy), v = fma(a1x, dx, a1y * dy);  |u| <= 0.5, |v| <= 0.5,
//     cg = 2^((u u + v v) * -46.16624) >= 0.0001.
// The device evaluates 2^x with v_exp_f32 (1 ulp) and may contract u u + v v into an fma: a pixel counts as accepted here when the smaller of the
// two forms of the sum gives cg >= 0.0001 (1 - SLACK), SLACK = 8 ulp.  Every accepted pixel must lie inside the new rectangle.
//
// Sets: (optional, argv[1]) quads of the benchmark's distribution, ten floats each — e0x e0y e1x e1y s0 s1 sx sy cx cy — for which the share of
// list entries and candidate pixels saved is printed; 10^6 seeded records at 1920 x 1080: rotations in steps of 1 degree (every other one
// jittered), anisotropy 1 .. 10^4 and footprints 0.01 .. 16 px log-uniform, both signs of sx and sy, centres anywhere, on pixel corners, on
// pixel centres, on tile corners and outside the image; 720 more with footprints 16 .. 2000 px (two per degree).
#include "../4dgaussiansplatrendering_amd/csrc/footprint_rect.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace {

constexpr int TILE = 8;
constexpr float SLACK = 8.0f * 0x1p-23f;

struct Quad { float e0x, e0y, e1x, e1y, s0, s1, sx, sy, cx, cy; };
struct Tally { uint64_t records = 0, old_entries = 0, new_entries = 0, old_pixels = 0, new_pixels = 0, accepted = 0, violations = 0, tightened = 0; };

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t next_u64() { uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
double uniform() { return (double)(next_u64() >> 11) * (1.0 / 9007199254740992.0); }
double log_uniform(double lo, double hi) { return lo * std::exp(uniform() * std::log(hi / lo)); }

uint64_t tiles_of(uint32_t r0, uint32_t r1) {
    const uint32_t x0 = r0 & 0xFFFFu, y0 = r0 >> 16, x1 = r1 & 0xFFFFu, y1 = r1 >> 16;
    if (x0 > x1 || y0 > y1) return 0;
    return (uint64_t)(x1 / TILE - x0 / TILE + 1u) * (y1 / TILE - y0 / TILE + 1u);
}
uint64_t pixels_of(uint32_t r0, uint32_t r1) {
    const uint32_t x0 = r0 & 0xFFFFu, y0 = r0 >> 16, x1 = r1 & 0xFFFFu, y1 = r1 >> 16;
    if (x0 > x1 || y0 > y1) return 0;
    return (uint64_t)(x1 - x0 + 1u) * (y1 - y0 + 1u);
}

void check(const Quad& q, int W, int H, Tally& t) {
    // emit(), csrc/preprocess.hip
    const float r0 = 1.0f / q.s0, r1 = 1.0f / q.s1;
    const float a0x = (q.e0x * r0) / q.sx, a0y = (q.e0y * r0) / q.sy;
    const float a1x = (q.e1x * r1) / q.sx, a1y = (q.e1y * r1) / q.sy;
    const float hx = 0.5f * (fabsf(q.e0x) * q.s0 + fabsf(q.e1x) * q.s1) * fabsf(q.sx);
    const float hy = 0.5f * (fabsf(q.e0y) * q.s0 + fabsf(q.e1y) * q.s1) * fabsf(q.sy);
    if (!(std::isfinite(q.cx) && std::isfinite(q.cy) && std::isfinite(a0x) && std::isfinite(a0y) && std::isfinite(a1x) && std::isfinite(a1y) && std::isfinite(hx) && std::isfinite(hy))) return;
    const float mx = 0.01f + 1e-5f * hx, my = 0.01f + 1e-5f * hy;
    uint32_t o0, o1, n0, n1;
    gs4d_footprint::pixel_rect(q.cx, q.cy, hx, hy, mx, my, W, H, o0, o1);
    float tx = hx, ty = hy;
    gs4d_footprint::tighten(q.e0x, q.e0y, q.e1x, q.e1y, q.s0, q.s1, q.sx, q.sy, tx, ty);
    gs4d_footprint::pixel_rect(q.cx, q.cy, tx, ty, mx, my, W, H, n0, n1);
    ++t.records;
    t.tightened += (tx < hx || ty < hy) ? 1u : 0u;
    t.old_entries += tiles_of(o0, o1); t.new_entries += tiles_of(n0, n1);
    t.old_pixels += pixels_of(o0, o1); t.new_pixels += pixels_of(n0, n1);
    if (pixels_of(o0, o1) == 0) return;
    const bool none = pixels_of(n0, n1) == 0;
    const int nx0 = (int)(n0 & 0xFFFFu), ny0 = (int)(n0 >> 16), nx1 = (int)(n1 & 0xFFFFu), ny1 = (int)(n1 >> 16);
    for (int y = (int)(o0 >> 16); y <= (int)(o1 >> 16); ++y) {
        const float fy = (float)y + 0.5f, dy = fy - q.cy;
        const float t0 = a0y * dy, t1 = a1y * dy;
        for (int x = (int)(o0 & 0xFFFFu); x <= (int)(o1 & 0xFFFFu); ++x) {
            const float fx = (float)x + 0.5f, dx = fx - q.cx;
            const float u = fmaf(a0x, dx, t0), v = fmaf(a1x, dx, t1);
            if (!(fabsf(u) <= 0.5f && fabsf(v) <= 0.5f)) continue;
            const float plain = u * u + v * v, fused = fmaf(u, u, v * v);
            const float cg = exp2f(fminf(plain, fused) * -46.16624130844683f);
            if (!(cg >= 0.0001f * (1.0f - SLACK))) continue;
            ++t.accepted;
            if (none || x < nx0 || x > nx1 || y < ny0 || y > ny1) {
                if (t.violations++ < 10)
                    fprintf(stderr, "accepted pixel (%d, %d) outside the new rectangle [%d, %d] x [%d, %d]: e0 = (%g, %g), s = (%g, %g), sx, sy = (%g, %g), c = (%g, %g), u, v = (%g, %g), cg = %g\n",
                            x, y, nx0, nx1, ny0, ny1, (double)q.e0x, (double)q.e0y, (double)q.s0, (double)q.s1, (double)q.sx, (double)q.sy, (double)q.cx, (double)q.cy, (double)u, (double)v, (double)cg);
            }
        }
    }
}

// a seeded quad: rotation `deg` degrees, anisotropy k, major half extent f pixels, centre of kind `kind`
Quad seeded(double deg, double k, double f, int kind, int W, int H) {
    const double th = deg * 3.14159265358979323846 / 180.0;
    Quad q;
    q.e0x = (float)std::cos(th); q.e0y = (float)std::sin(th);
    q.e1x = q.e0y; q.e1y = -q.e0x;                                    // as eigen2 builds the second axis
    const double sxm = 200.0 + 1500.0 * uniform();                    // window scale, both signs
    q.sx = (float)((next_u64() & 1u) ? sxm : -sxm);
    q.sy = (float)((next_u64() & 1u) ? sxm : -sxm);
    const double major = 2.0 * f / sxm, minor = major / k;            // the quad reaches 0.5 * s along an axis
    if (next_u64() & 1u) { q.s0 = (float)minor; q.s1 = (float)major; } else { q.s0 = (float)major; q.s1 = (float)minor; }
    double cx = uniform() * W, cy = uniform() * H;
    switch (kind) {
    case 1: cx = std::floor(cx); cy = std::floor(cy); break;                        // pixel corners
    case 2: cx = std::floor(cx) + 0.5; cy = std::floor(cy) + 0.5; break;            // pixel centres
    case 3: cx = std::floor(cx / TILE) * TILE; cy = std::floor(cy / TILE) * TILE; break;      // tile corners
    case 4: {                                                                       // outside the image, within reach of it or not
        const double out = (f + 1.0) * 1.2 * uniform();
        switch (next_u64() & 3u) { case 0: cx = -out; break; case 1: cx = W + out; break; case 2: cy = -out; break; default: cy = H + out; break; }
        break;
    }
    default: break;
    }
    q.cx = (float)cx; q.cy = (float)cy;
    return q;
}

void report(const char* name, const Tally& t) {
    printf("%s: %llu records (%llu tightened), entries %llu -> %llu (%.2f %% saved), candidate pixels %llu -> %llu (%.2f %% saved), %llu accepted pixels, %llu violations\n", name,
           (unsigned long long)t.records, (unsigned long long)t.tightened, (unsigned long long)t.old_entries, (unsigned long long)t.new_entries,
           t.old_entries ? 100.0 * (double)(t.old_entries - t.new_entries) / (double)t.old_entries : 0.0, (unsigned long long)t.old_pixels, (unsigned long long)t.new_pixels,
           t.old_pixels ? 100.0 * (double)(t.old_pixels - t.new_pixels) / (double)t.old_pixels : 0.0, (unsigned long long)t.accepted, (unsigned long long)t.violations);
}

} // namespace

int main(int argc, char** argv) {
    const int W = 1920, H = 1080;
    uint64_t bad = 0;
    if (argc > 1) {
        FILE* f = fopen(argv[1], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
        std::vector<Quad> quads;
        Quad q;
        while (fread(&q, sizeof q, 1, f) == 1) quads.push_back(q);
        fclose(f);
        Tally t;
        for (const Quad& k : quads) check(k, W, H, t);
        report("benchmark", t);
        bad += t.violations;
        if (t.records == 0) { fprintf(stderr, "no valid record in %s\n", argv[1]); return 2; }
    }
    {
        Tally t;
        const uint32_t n = 1000000u;
        for (uint32_t i = 0; i < n; ++i) {
            const double deg = (double)(i % 360u) + ((i / 360u) & 1u ? uniform() : 0.0);
            check(seeded(deg, log_uniform(1.0, 1e4), log_uniform(0.01, 16.0), (int)((i / 720u) % 5u), W, H), W, H, t);
        }
        report("seeded, 0.01 .. 16 px", t);
        bad += t.violations;
        if (t.records != n || t.accepted == 0 || t.tightened < n / 4) { fprintf(stderr, "the seeded set shows nothing\n"); return 2; }
    }
    {
        Tally t;
        const uint32_t n = 720u;
        for (uint32_t i = 0; i < n; ++i) check(seeded((double)(i % 360u), log_uniform(1.0, 1e4), log_uniform(16.0, 2000.0), (int)((i / 360u + i) % 5u), W, H), W, H, t);
        report("seeded, 16 .. 2000 px", t);
        bad += t.violations;
        if (t.records != n || t.accepted == 0) { fprintf(stderr, "the large set shows nothing\n"); return 2; }
    }
    return bad ? 1 : 0;
}
