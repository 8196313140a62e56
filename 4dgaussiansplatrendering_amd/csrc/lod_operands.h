// lod_operands.h — the argument checks of gs4d_lod_append and gs4d_lod_cut that need no context (include/gs4d.h): the scalar rule of an append and
// the two calls' operand lists (operands.h), declared once.  gs4d_api.hip refuses a call by them and queues its kernels from the same lists;
// tests/lod_query_check.cpp runs them on the CPU over a table of buffers of its own.  Plain C++17: no HIP type, no context.
#pragma once
#include "operands.h"

namespace gs4d {

constexpr int LOD_APPEND_OPERANDS = 4, LOD_CUT_OPERANDS = 6;

// why gs4d_lod_append refuses its numbers, or null
inline const char* lod_append_fault(uint64_t m, bool member_group_given, uint64_t child_first, uint64_t c, uint64_t first) {
    if (m > 0xFFFFFFFEull || first > 0xFFFFFFFEull || first + m > 0xFFFFFFFEull) return "first + m above 2^32 - 2";
    if (child_first > first || c > first - child_first) return "child_first + c above first: a child lies below its parent's level";
    if (!member_group_given && c != 0) return "c != 0 without member_group";
    return nullptr;
}
// level and member_group are read; nodes is written as gs4d_transform_records writes a dst with dst_first; parent is a kernel write that keeps the
// rest of its contents (child_first + c <= first: first + m rows cover the children's words)
inline void lod_append_operands(Operand (&op)[LOD_APPEND_OPERANDS], uint32_t level, uint64_t m, uint32_t member_group, uint64_t c, uint32_t nodes,
                                uint32_t parent, uint64_t first) {
    op[0] = Operand{ "level", level, false, 96, m, OP_READ };
    op[1] = Operand{ "member_group", member_group, true, sizeof(uint32_t), c, OP_READ };
    op[2] = Operand{ "nodes", nodes, false, 96, first + m, OP_WRITE };
    op[3] = Operand{ "parent", parent, false, sizeof(uint32_t), first + m, OP_WRITE };
}
// nodes and parent are read (the 96-byte records, never a shadow: a reader leaves `version` alone); dst is written as gs4d_transform_records writes
// its own and holds what it holds, like cut_index; stats as in gs4d_count_centres: a read-modify-write the lane has the table to itself for; count
// is written whole
inline void lod_cut_operands(Operand (&op)[LOD_CUT_OPERANDS], uint32_t nodes, uint32_t parent, uint64_t n, uint32_t dst, uint32_t cut_index,
                             uint32_t stats, uint32_t count) {
    op[0] = Operand{ "nodes", nodes, false, 96, n, OP_READ };
    op[1] = Operand{ "parent", parent, false, sizeof(uint32_t), n, OP_READ };
    op[2] = Operand{ "dst", dst, true, 96, 0, OP_WRITE };
    op[3] = Operand{ "cut_index", cut_index, true, sizeof(uint32_t), 0, OP_WRITE };
    op[4] = Operand{ "stats", stats, true, 16, n, OP_WRITE | OP_SETTLE };
    op[5] = Operand{ "count", count, false, 1, 16, OP_WRITE };
}

} // namespace gs4d
