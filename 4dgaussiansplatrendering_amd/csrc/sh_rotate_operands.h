// sh_rotate_operands.h — the argument checks of gs4d_rotate_sh that need no context (include/gs4d.h): its scalar rules and its operand list
// (operands.h), declared once.  gs4d_api.hip refuses a call by them and queues its kernel from the same list; host/gs4d_host.cpp refuses by the same
// scalar rules; tests/sh_rotate_check.cpp runs them on the CPU over a table of buffers of its own.  Plain C++17: no HIP type, no context.
#pragma once
#include "operands.h"

namespace gs4d {

constexpr int ROTATE_SH_OPERANDS = 4;
// the forms (GS4D_POSE_INDEX, GS4D_POSE_BLEND4 and GS4D_SH_EACH of gs4d.h: gs4d_api.hip asserts that they are these)
constexpr uint32_t SHROT_INDEX = 0u, SHROT_BLEND4 = 1u, SHROT_EACH = 2u;

// rows of dst the call writes, from dst_first on (the numbers already checked: no overflow)
inline uint64_t rotate_sh_rows(uint64_t n, uint64_t m, uint32_t form) { return form == SHROT_EACH ? n * m : n; }

// why gs4d_rotate_sh refuses its numbers, or null
inline const char* rotate_sh_fault(uint64_t n, uint64_t stride, int degree, uint64_t m, bool bind_given, uint32_t form, uint64_t bind_stride, uint64_t dst_first) {
    if (n > 0xFFFFFFFFull || m > 0xFFFFFFFFull || dst_first > 0xFFFFFFFFull) return "n, m or dst_first above 2^32 - 1";
    if (degree < 0 || degree > 3) return "degree must be 0, 1, 2 or 3";
    if (stride < 16 || stride > 1024 || stride % 16 != 0) return "stride must be a multiple of 16 from 16 to 1024";
    if (stride < 12u * (uint64_t)((degree + 1) * (degree + 1))) return "stride holds fewer than 12 (degree + 1)^2 bytes";
    if (form != SHROT_INDEX && form != SHROT_BLEND4 && form != SHROT_EACH) return "form is none of GS4D_POSE_INDEX, GS4D_POSE_BLEND4, GS4D_SH_EACH";
    if (form == SHROT_EACH) {
        if (bind_given) return "bind must be 0 with GS4D_SH_EACH";
    } else {
        if (!bind_given) return "bind is 0: GS4D_POSE_INDEX and GS4D_POSE_BLEND4 need a bind table";
        if (form == SHROT_INDEX && (bind_stride < 4 || bind_stride % 4 != 0)) return "bind_stride must be a multiple of 4, at least 4";
        if (form == SHROT_BLEND4 && (bind_stride < 32 || bind_stride % 16 != 0)) return "bind_stride must be a multiple of 16, at least 32";
    }
    const uint64_t total = rotate_sh_rows(n, m, form);             // (both factors below 2^32: no overflow)
    if (total > 0xFFFFFFFFull || dst_first + total > 0xFFFFFFFFull) return form == SHROT_EACH ? "dst_first + m * n above 2^32 - 1" : "dst_first + n above 2^32 - 1";
    return nullptr;
}

// src, xf and bind (not given with GS4D_SH_EACH) are read; dst is a kernel write that keeps the rows the call does not name.  A table is no record
// buffer: there is no shadow to build or to drop.
inline void rotate_sh_operands(Operand (&op)[ROTATE_SH_OPERANDS], uint32_t src, uint64_t n, uint64_t stride, uint32_t xf, uint64_t m, uint32_t bind, uint32_t form,
                               uint64_t bind_stride, uint32_t dst, uint64_t dst_first) {
    const bool each = form == SHROT_EACH;
    op[0] = Operand{ "src", src, false, (size_t)stride, n, OP_READ };
    op[1] = Operand{ "xf", xf, false, 80, m, OP_READ };
    op[2] = Operand{ "bind", bind, each, each ? (size_t)1 : (size_t)bind_stride, each ? 0 : n, OP_READ };
    op[3] = Operand{ "dst", dst, false, (size_t)stride, dst_first + rotate_sh_rows(n, m, form), OP_WRITE };
}

} // namespace gs4d
