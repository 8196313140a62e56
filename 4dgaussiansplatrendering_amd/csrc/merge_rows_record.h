// merge_rows_record.h — the arithmetic of gs4d_merge_rows (include/gs4d.h) as plain C++ inline functions: the one text of the
// definition.  csrc/merge_rows.hip evaluates the word functions on the device, host/gs4d_host.cpp (gs4d_host_merge_rows) and
// tests/merge_rows_check.cpp run the loop below on the CPU.  The weight of a record is member_mass of merge_record.h; the sums of a group live in the
// eight interleaved slots of that header, combined by its tree, for the reason given there.  Build without contraction; the division is correctly
// rounded.
#ifndef GS4D_MERGE_ROWS_RECORD_H
#define GS4D_MERGE_ROWS_RECORD_H

#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "merge_record.h"

namespace gs4d_rows {

constexpr int SLOTS = gs4d_merge::SLOTS;
constexpr uint32_t NONE = gs4d_merge::NONE;

// the stride rule of gs4d_shade_sh, and the query of gs4d_merge_rows
GS4D_HD inline bool stride_ok(uint64_t stride) { return stride >= 16u && stride <= 1024u && stride % 16u == 0u; }
GS4D_HD inline bool query_ok(uint32_t stride, uint32_t width, uint32_t flags, uint32_t reserved) {
    return stride_ok(stride) && width != 0u && (uint64_t)4u * width <= stride && flags == 0u && reserved == 0u;
}
// a_i and ok_i: the mass of gs4d_merge_records for a record, 1 without records
GS4D_HD inline bool weight(const float* rec, float& a) {
    if (!rec) { a = 1.0f; return true; }
    return gs4d_merge::member_mass(rec, a);
}
// what a word of a member's row adds to its sum, and the word of a larger group from its combined sums
GS4D_HD inline double term(double a, float word) { return a * (double)word; }
GS4D_HD inline float quotient(double r, double w) { return (float)(r / w); }

// whether words 0 .. width - 1 of a row are all finite
inline bool row_finite(const float* row, uint32_t width) {
    for (uint32_t j = 0; j < width; ++j) if (!gs4d_merge::finite(row[j])) return false;
    return true;
}

// The definition as one loop on one thread.  rec: n records of 24 floats, or null: unit weights.  rows: n rows of `stride` bytes.  dst: `capacity`
// rows of `stride` bytes.  count: {groups, written, members, left_out}.  A query the device call refuses writes nothing.
inline void host_merge_rows(size_t n, const float* rec, const uint32_t* member_group, const void* rows, uint32_t stride, uint32_t width, uint32_t flags,
                            uint32_t reserved, void* dst, size_t dst_first, size_t capacity, uint32_t count[4]) {
    if (!query_ok(stride, width, flags, reserved) || n > 0xFFFFFFFEull || dst_first > 0xFFFFFFFEull) return;
    const unsigned char* const src = (const unsigned char*)rows;
    auto row_of = [&](uint32_t i, float* to) { memcpy(to, src + (size_t)i * stride, 4u * (size_t)width); };
    std::vector<uint32_t> member;
    std::vector<float> row(width);
    for (size_t i = 0; i < n; ++i) {
        float a;
        if (member_group[i] == NONE || !weight(rec ? rec + 24 * i : nullptr, a)) continue;
        row_of((uint32_t)i, row.data());
        if (row_finite(row.data(), width)) member.push_back((uint32_t)i);
    }
    std::stable_sort(member.begin(), member.end(), [member_group](uint32_t x, uint32_t y) { return member_group[x] < member_group[y]; });
    uint32_t groups = 0, written = 0;
    std::vector<double> R((size_t)SLOTS * width);
    std::vector<float> out(stride / 4u);
    for (size_t first = 0, end; first < member.size(); first = end, ++groups) {
        const uint32_t g = member_group[member[first]];
        for (end = first + 1; end < member.size() && member_group[member[end]] == g; ++end) {}
        if ((uint64_t)dst_first + g >= (uint64_t)capacity) continue;
        ++written;
        std::fill(out.begin(), out.end(), 0.0f);
        if (end - first == 1) {
            row_of(member[first], out.data());
        } else {
            double W[SLOTS];
            for (int s = 0; s < SLOTS; ++s) W[s] = 0.0;
            std::fill(R.begin(), R.end(), 0.0);
            for (size_t k = first; k < end; ++k) {
                const uint32_t i = member[k];
                const int s = (int)((k - first) % SLOTS);
                float a;
                (void)weight(rec ? rec + 24 * (size_t)i : nullptr, a);
                row_of(i, row.data());
                W[s] += (double)a;
                for (uint32_t j = 0; j < width; ++j) R[(size_t)s * width + j] += term((double)a, row[j]);
            }
            for (int step = 1; step < SLOTS; step <<= 1)
                for (int s = 0; s < SLOTS; s += 2 * step) {
                    W[s] += W[s + step];
                    for (uint32_t j = 0; j < width; ++j) R[(size_t)s * width + j] += R[(size_t)(s + step) * width + j];
                }
            for (uint32_t j = 0; j < width; ++j) out[j] = quotient(R[j], W[0]);
        }
        memcpy((unsigned char*)dst + ((size_t)dst_first + g) * stride, out.data(), stride);
    }
    count[0] = groups; count[1] = written; count[2] = (uint32_t)member.size(); count[3] = (uint32_t)(n - member.size());
}

} // namespace gs4d_rows
#endif
