// Host side of the resident pendulum kernel's completion line (kernels_fused.hpp, the kernel's tail): plain C++, no HIP.
//
// One 64-byte line (16 words) per agent in pinned host memory.  Words 0..9 carry the ten half-words of the packed record
// (action | next state[3] | reward): word 2f = (low half of float f) << 16 | tag, word 2f+1 = (high half of float f) << 16
// | tag, where tag = the low 16 bits of the call's sequence number.  Words 10..14 carry the tag alone and are not looked
// at; word 15 carries the whole sequence number.  The GPU stores the words relaxed, in no particular order: the line
// is accepted only when words 0..9 AND word 15 all name the awaited call, so a line caught half-written -- some words
// still from an earlier call -- is refused and read again.  (The request line of Engine::resident_step, mirrored.)
#pragma once
#include <cstdint>
#include <cstring>

namespace bbmpc {

constexpr int kCompletionRecordFloats = 5;       // U + S + 1 of the pendulum record (U = 1, S = 3)

// true: every word names `seq`, rec[0..4] holds the record bit for bit.  false: rec is untouched.
inline bool completion_line_decode(const volatile uint32_t* line, uint32_t seq, float* rec) {
    if (line[15] != seq) return false;            // (the one word a spinning caller reads per poll)
    uint32_t w[2 * kCompletionRecordFloats];
    for (int i = 0; i < 2 * kCompletionRecordFloats; ++i) w[i] = line[i];
    const uint32_t tag = seq & 0xffffu;
    for (int i = 0; i < 2 * kCompletionRecordFloats; ++i)
        if ((w[i] & 0xffffu) != tag) return false;
    for (int f = 0; f < kCompletionRecordFloats; ++f) {
        const uint32_t bits = (w[2 * f] >> 16) | (w[2 * f + 1] & 0xffff0000u);
        memcpy(rec + f, &bits, 4);
    }
    return true;
}

// what the kernel stores (the tests' and the host's way to write a line: never used on the hot path)
inline void completion_line_encode(uint32_t* line, uint32_t seq, const float* rec) {
    const uint32_t tag = seq & 0xffffu;
    for (int f = 0; f < kCompletionRecordFloats; ++f) {
        uint32_t bits;
        memcpy(&bits, rec + f, 4);
        line[2 * f] = (bits << 16) | tag;
        line[2 * f + 1] = (bits & 0xffff0000u) | tag;
    }
    for (int i = 2 * kCompletionRecordFloats; i < 15; ++i) line[i] = tag;
    line[15] = seq;
}

}  // namespace bbmpc
