// merge_record_check — the text of gs4d_cell_labels and gs4d_merge_records (csrc/merge_record.h, what csrc/merge.hip evaluates on the device and the
// host library on the CPU) compiled stand-alone: tests/test_merge_host.py builds this with `g++ -O2 -std=c++17 -ffp-contract=off` (and once more with
// -fsanitize=address,undefined) and compares its output with gs4d_host_merge_records and gs4d_host_cell_labels, word for word.  Both sides are the
// same text, so this checks the flags and the compilers: another compiler gives the library's bits.  The buffers are allocated at exactly the sizes
// the definitions demand, so the instrumented build also shows that nothing past record, label or row n - 1 is read.
//
//   merge_record_check merge N ALPHA_MAX_BITS IN LABELS KEEP OUT GROUPS MEMBER_GROUP COUNT
//   merge_record_check cells N IN GRID OUT
// IN: N records of 24 float32.  LABELS: N uint32.  KEEP: N bytes, non-zero where the record's table row passes the rule.  ALPHA_MAX_BITS: the bits
// of alpha_max in decimal.  OUT / GROUPS: one 96-byte record / one {label, size, first, 0} row per group.  MEMBER_GROUP: N uint32.  COUNT: {groups,
// written, members, left_out}.  GRID: the 64 bytes of a gs4d_cell_grid that the call takes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../4dgaussiansplatrendering_amd/csrc/merge_record.h"

namespace mg = gs4d_merge;

struct Grid { float lo[4], edge[4]; uint32_t dims[4], reserved[4]; };            // gs4d_cell_grid
static_assert(sizeof(Grid) == 64, "the structure of include/gs4d.h");

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

static int cells(int argc, char** argv) {
    if (argc != 6) return 2;
    const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
    std::vector<float> rec(n * 24);
    std::vector<uint32_t> labels(n);
    Grid g;
    if (!slurp(argv[3], rec.data(), n * 96) || !slurp(argv[4], &g, sizeof g)) return 1;
    if (!mg::grid_ok(g.edge, g.dims, g.reserved)) { std::fprintf(stderr, "a grid the call refuses\n"); return 2; }
    for (size_t i = 0; i < n; ++i) labels[i] = mg::cell_label(g.lo, g.edge, g.dims, &rec[24 * i]);
    return spill(argv[5], labels.data(), n * 4) ? 0 : 1;
}

static int merge(int argc, char** argv) {
    if (argc != 11) return 2;
    const size_t n = (size_t)std::strtoull(argv[2], nullptr, 10);
    const uint32_t alpha_bits = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    float alpha_max;
    std::memcpy(&alpha_max, &alpha_bits, 4);
    if (!(mg::finite(alpha_max) && alpha_max > 0.0f) || n >= 0xFFFFFFFFull) { std::fprintf(stderr, "a call the library refuses\n"); return 2; }
    std::vector<float> rec(n * 24);
    std::vector<uint32_t> labels(n), member_group(n, mg::NONE), member;
    std::vector<unsigned char> keep(n);
    if (!slurp(argv[4], rec.data(), n * 96) || !slurp(argv[5], labels.data(), n * 4) || !slurp(argv[6], keep.data(), n)) return 1;
    for (size_t i = 0; i < n; ++i) {
        float a;
        if (labels[i] != mg::NONE && keep[i] && mg::member_mass(&rec[24 * i], a)) member.push_back((uint32_t)i);
    }
    std::stable_sort(member.begin(), member.end(), [&](uint32_t x, uint32_t y) { return labels[x] < labels[y]; });
    std::vector<float> out;
    std::vector<uint32_t> rows;
    uint32_t g = 0;
    for (size_t first = 0, end; first < member.size(); first = end, ++g) {
        const uint32_t label = labels[member[first]];
        for (end = first + 1; end < member.size() && labels[member[end]] == label; ++end) {}
        float o[24];
        const float* const origin = &rec[24 * (size_t)member[first]];
        if (end - first == 1) {
            std::memcpy(o, origin, 96);
        } else {
            mg::Sums slot[mg::SLOTS];
            for (int s = 0; s < mg::SLOTS; ++s) mg::clear(slot[s]);
            for (size_t k = first; k < end; ++k) {
                const float* const r = &rec[24 * (size_t)member[k]];
                float a;
                (void)mg::member_mass(r, a);
                mg::add_member(slot[(k - first) % mg::SLOTS], origin, a, r);
            }
            mg::join_slots(slot);
            mg::finish(slot[0], origin, alpha_max, o);
        }
        out.insert(out.end(), o, o + 24);
        const uint32_t row[4] = { label, (uint32_t)(end - first), member[first], 0u };
        rows.insert(rows.end(), row, row + 4);
        for (size_t k = first; k < end; ++k) member_group[member[k]] = g;
    }
    const uint32_t count[4] = { g, g, (uint32_t)member.size(), (uint32_t)(n - member.size()) };
    return spill(argv[7], out.data(), out.size() * 4) && spill(argv[8], rows.data(), rows.size() * 4) && spill(argv[9], member_group.data(), n * 4) &&
           spill(argv[10], count, 16) ? 0 : 1;
}

int main(int argc, char** argv) {
    int rc = 2;
    if (argc >= 2 && std::strcmp(argv[1], "merge") == 0) rc = merge(argc, argv);
    else if (argc >= 2 && std::strcmp(argv[1], "cells") == 0) rc = cells(argc, argv);
    if (rc == 2) std::fprintf(stderr, "usage: merge_record_check merge N ALPHA_MAX_BITS IN LABELS KEEP OUT GROUPS MEMBER_GROUP COUNT | cells N IN GRID OUT\n");
    return rc;
}
