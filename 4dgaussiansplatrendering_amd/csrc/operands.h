// The buffer arguments of a record-set call, declared once: what each is called, whether it may be left out, how many rows of how many bytes it
// must hold, and what the call does with it.  gs4d_api.hip checks a call's list with check_operand_list and queues its kernels from the same
// list (check_operands, queue_operands); tests/operand_check.cpp runs the check on the CPU.  Plain C++17: no HIP type, no context.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace gs4d {

// what a call does with an operand (any combination; none: the operand is only checked)
enum : unsigned {
    OP_READ = 1u,      // the kernels read it: the lane waits for its last writer
    OP_WRITE = 2u,     // the kernels write it (or read-modify-write it): the lane waits for its writer and its readers, pending draws that may be
                       // re-run from it are settled first, its version moves on and its provenance is dropped
    OP_SETTLE = 4u,    // a statistics table draws may have added to: every draw issued so far is behind it before anything is queued
    OP_SCAN = 8u       // a statistics table draws may still add to while the kernels read it: they leave an event behind for those draws
};

struct Operand {
    const char* arg;       // the argument's name as the messages spell it
    uint32_t name;         // the gs4d_buf
    bool optional;         // 0 means "not given"
    size_t row;            // bytes per row; 1: `rows` is a byte count
    uint64_t rows;         // rows the buffer must hold (a sum such as dst_first + m * n stays 64-bit)
    unsigned roles;        // OP_*
};

struct BufferFacts { bool live; size_t bytes; };      // what the check needs to know of a name

enum class OperandFault { None, Missing, NotLive, Same, Short };
struct OperandVerdict { OperandFault fault; int at, other; };      // ops[at] is at fault; Same: it names the buffer ops[other] names

// lookup(name) -> BufferFacts, asked for non-zero names only.  A required name is non-zero and live, an optional one 0 or live; no two non-zero names
// are equal; every given buffer holds its rows (bytes / row < rows: no product, no overflow).  The names are all decided before any size.
template <class Lookup>
OperandVerdict check_operand_list(const Operand* ops, int count, Lookup lookup) {
    for (int i = 0; i < count; ++i) {
        if (ops[i].name == 0u) { if (!ops[i].optional) return { OperandFault::Missing, i, -1 }; continue; }
        if (!lookup(ops[i].name).live) return { OperandFault::NotLive, i, -1 };
        for (int j = 0; j < i; ++j) if (ops[j].name == ops[i].name) return { OperandFault::Same, i, j };
    }
    for (int i = 0; i < count; ++i)
        if (ops[i].name != 0u && lookup(ops[i].name).bytes / ops[i].row < ops[i].rows) return { OperandFault::Short, i, -1 };
    return { OperandFault::None, -1, -1 };
}

// "<fn>: <operand> ..." for a verdict other than None
inline std::string operand_message(const char* fn, const Operand* ops, const OperandVerdict& v) {
    const Operand& o = ops[v.at];
    std::string m = std::string(fn) + ": " + o.arg;
    switch (v.fault) {
    case OperandFault::Missing: return m + " is 0: the call needs this buffer";
    case OperandFault::NotLive: return m + " (" + std::to_string(o.name) + ") is not a live buffer";
    case OperandFault::Same:    return m + " and " + ops[v.other].arg + " must be different buffers";
    case OperandFault::Short:   return m + " holds fewer than " + std::to_string(o.rows) + (o.row == 1 ? " bytes" : " rows of " + std::to_string(o.row) + " bytes");
    default:                    return m;
    }
}

} // namespace gs4d
