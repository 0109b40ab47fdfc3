// Where the slots of one host call's staging buffer lie (abi_util.hpp: HostStage).  Plain C++ without HIP, so that a CPU
// program can check the arithmetic (tests/host_stage_layout_check.cpp).
#pragma once
#include <stddef.h>
#include <stdexcept>

namespace bbmpc {

// Slots in declaration order, disjoint and packed back to back; a slot that asks for it starts at a multiple of `align`
// floats (kVec4: 16 bytes from the buffer's 256-byte aligned base, for float4 traffic).  A slot that is not wanted -- an
// optional argument the caller left NULL -- or that has no elements takes no space and resolves to a null pointer.
struct StageLayout {
    static constexpr size_t kVec4 = 4, kNone = ~(size_t)0;
    static constexpr int kMaxSlots = 16;
    size_t off[kMaxSlots], len[kMaxSlots];
    int n = 0;
    size_t total = 0;              // floats the buffer has to hold: the end of the last slot that takes space
    int add(size_t count, bool wanted = true, size_t align = 1) {
        if (n == kMaxSlots) throw std::logic_error("internal: a host call stages more than 16 tensors");
        len[n] = wanted ? count : 0;
        off[n] = len[n] ? (total + align - 1) / align * align : kNone;
        if (len[n]) total = off[n] + len[n];
        return n++;
    }
    template <class T>
    T* at(T* base, int slot) const { return off[slot] == kNone ? nullptr : base + off[slot]; }
};

}  // namespace bbmpc
