// rows_operands.h — the argument checks of gs4d_merge_rows and gs4d_copy_rows that need no context (include/gs4d.h): their scalar rules and their
// operand lists (operands.h), declared once.  gs4d_api.hip refuses a call by them and queues its kernels from the same lists;
// tests/merge_rows_check.cpp runs them on the CPU over a table of buffers of its own.  Plain C++17: no HIP type, no context.
#pragma once
#include "operands.h"

namespace gs4d {

constexpr int MERGE_ROWS_OPERANDS = 5, COPY_ROWS_OPERANDS = 2;

inline bool rows_stride_ok(uint64_t stride) { return stride >= 16 && stride <= 1024 && stride % 16 == 0; }

// why gs4d_merge_rows refuses its numbers, or null (query_given: q != NULL; the four words: the query's)
inline const char* merge_rows_fault(bool query_given, uint32_t stride, uint32_t width, uint32_t flags, uint32_t reserved, uint64_t n, uint64_t dst_first) {
    if (!query_given) return "q == NULL";
    if (!rows_stride_ok(stride)) return "stride must be a multiple of 16 from 16 to 1024";
    if (width == 0 || (uint64_t)4 * width > stride) return "width must be 1 .. stride / 4";
    if (flags != 0 || reserved != 0) return "flags or the reserved field of the query is not 0";
    if (n > 0xFFFFFFFEull) return "the sort takes 2^32 - 2 records at most";
    if (dst_first > 0xFFFFFFFEull) return "dst_first above 2^32 - 2";
    return nullptr;
}
// data (optional: unit weights), member_group and rows are read (the 96-byte records, never a shadow: a reader leaves `version` alone); dst is a
// kernel write that keeps the rows the call does not name and holds what it holds (the capacity); count is written whole
inline void merge_rows_operands(Operand (&op)[MERGE_ROWS_OPERANDS], uint32_t data, uint64_t n, uint32_t member_group, uint32_t rows, uint32_t stride,
                                uint32_t dst, uint32_t count) {
    op[0] = Operand{ "data", data, true, 96, n, OP_READ };
    op[1] = Operand{ "member_group", member_group, false, sizeof(uint32_t), n, OP_READ };
    op[2] = Operand{ "rows", rows, false, stride, n, OP_READ };
    op[3] = Operand{ "dst", dst, false, stride, 0, OP_WRITE };
    op[4] = Operand{ "count", count, false, 1, 16, OP_WRITE };
}

// why gs4d_copy_rows refuses its numbers, or null
inline const char* copy_rows_fault(uint64_t src_first, uint64_t m, uint64_t stride, uint64_t dst_first) {
    if (!rows_stride_ok(stride)) return "stride must be a multiple of 16 from 16 to 1024";
    if (m > 0xFFFFFFFFull || src_first > 0xFFFFFFFFull || dst_first > 0xFFFFFFFFull) return "m, src_first or dst_first above 2^32 - 1";
    return nullptr;
}
// src is read, dst is a kernel write that keeps the rest of its contents (first + m <= 2^33: no wrap)
inline void copy_rows_operands(Operand (&op)[COPY_ROWS_OPERANDS], uint32_t src, uint64_t src_first, uint64_t m, uint64_t stride, uint32_t dst, uint64_t dst_first) {
    op[0] = Operand{ "src", src, false, (size_t)stride, src_first + m, OP_READ };
    op[1] = Operand{ "dst", dst, false, (size_t)stride, dst_first + m, OP_WRITE };
}

} // namespace gs4d
