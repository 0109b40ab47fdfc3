// The arithmetic of the radix select in topk.hpp -- the order-preserving key of a reward, the key range of a selection,
// the digit a key shows in a pass and whether the key takes part in it -- for the kernels and for a CPU program alike:
// plain C++, no HIP needed (tests/topk_digits_check.cpp runs the multi-pass loop serially from here).
//
// A selection works on OFFSET keys  key' = reward_key(r) - kmin  (unsigned 32-bit; kmin = the smallest key of the
// population, so the subtraction is exact and monotone for every key).  With B an upper bound of the k-th smallest key:
//     span = B - kmin,   top = bit_length(span)          (span == 0: at least k keys tie for best, no pass runs)
// Only keys with key' <= span can be among the k smallest; only they enter a histogram.  The first pass takes the
// TOPK_W1 bits below bit `top` of key' (all of them when top <= TOPK_W1), later passes the next TOPK_WN bits each.  The
// digit of a population that straddles a binade (-127.9 ... -128.1) therefore spreads over all the bins of the first
// pass; a digit taken below the highest bit in which kmin and B DIFFER would put it into two or three of them.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BBMPC_TOPK_HD __host__ __device__ __forceinline__
#else
#define BBMPC_TOPK_HD inline
#endif

namespace bbmpc {

constexpr int TOPK_W1 = 10;                         // bits of the first pass's digit
constexpr int TOPK_WN = 8;                          // bits of every later pass's digit
constexpr int TOPK_BINS1 = 1 << TOPK_W1;            // first histogram
constexpr int TOPK_BINSN = 1 << TOPK_WN;            // second histogram (later passes alternate between it and the first 256
                                                    // words of the first one)
// LDS words of a selection: second histogram | 16 control words | first histogram.  The per-wave (kmin, bound) slots of
// the key range live in the SECOND histogram's words [0, 16) and [16, 32): the first pass does not touch that array, and
// it is zeroed for pass 1 while pass 0 is scanned -- behind the barrier every wave has read the slots in front of.
// The first histogram lies last so that a caller short of LDS (the CMA-ES kernels, whose population limit is set by
// the words beside the rewards) can run the NARROW form: 8 bits in the first pass too, 256 words of first histogram,
// TOPK_HIST_WORDS_NARROW in all.  The selection is exact either way: the same elites, only more second passes.
constexpr int TOPK_HIST2_OFF = 0;
constexpr int TOPK_CTRL_OFF = TOPK_BINSN;
constexpr int TOPK_HIST1_OFF = TOPK_BINSN + 16;
constexpr int TOPK_HIST_WORDS = TOPK_BINSN + 16 + TOPK_BINS1;
constexpr int TOPK_HIST_WORDS_NARROW = TOPK_BINSN + 16 + TOPK_BINSN;
constexpr int TOPK_MAX_PASSES = 1 + (32 - TOPK_W1 + TOPK_WN - 1) / TOPK_WN;
static_assert(TOPK_W1 >= TOPK_WN && TOPK_W1 <= 10, "wave 0 scans the first histogram with 16 bins per lane at most");

// smaller key == better (larger reward); equal rewards <=> equal keys (-0 is folded onto +0 first)
BBMPC_TOPK_HD uint32_t reward_key(float r) {
    const float f = r + 0.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    const uint32_t u = __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
#endif
    const uint32_t asc = u ^ ((u >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    return ~asc;
}

BBMPC_TOPK_HD int topk_bit_length(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return x ? 32 - __clz((int)x) : 0;
#else
    return x ? 32 - __builtin_clz(x) : 0;
#endif
}

// the range of a selection: offset keys lie in [0, span] as far as they matter, `top` bits are undecided
struct TopkRange {
    uint32_t kmin;
    uint32_t span;
    int top;
};
BBMPC_TOPK_HD TopkRange topk_range(uint32_t kmin, uint32_t bound) {
    const uint32_t span = bound - kmin;
    return TopkRange{kmin, span, topk_bit_length(span)};
}

BBMPC_TOPK_HD uint32_t topk_offset_key(float r, uint32_t kmin) { return reward_key(r) - kmin; }

// pass `pass` with `top` undecided low bits: how many of them it decides, and what is left below them
// (w1: the first pass's bits, TOPK_W1 or, in the narrow form, TOPK_WN)
BBMPC_TOPK_HD int topk_pass_width(int pass, int top, int w1 = TOPK_W1) {
    const int w = pass == 0 ? w1 : TOPK_WN;
    return top < w ? top : w;
}
BBMPC_TOPK_HD int topk_pass_shift(int pass, int top, int w1 = TOPK_W1) { return top - topk_pass_width(pass, top, w1); }

// the digit of offset key kp in that pass (for a key that takes part)
BBMPC_TOPK_HD uint32_t topk_digit(uint32_t kp, int pass, int top, int w1 = TOPK_W1) {
    const int w = topk_pass_width(pass, top, w1);
    return (kp >> (top - w)) & ((1u << w) - 1u);
}

// does offset key kp enter the histogram of a pass?  T = the decided high bits of the k-th offset key (0 before the first
// pass), top = the number of undecided low bits (< 32 behind the first pass; 32 is possible in front of it, where every
// key within the span takes part)
BBMPC_TOPK_HD bool topk_takes_part(uint32_t kp, uint32_t span, uint32_t T, int top) {
    return kp <= span && (top >= 32 || (kp >> top) == (T >> top));
}

// LDS word of bin d in the FIRST histogram.  Wave 0 scans it with four 16-byte reads per lane, lane l reading vector
// q * 64 + l (q = 0..3: consecutive lanes, consecutive vectors, no bank conflict); those four vectors hold the 16
// consecutive bins 16 l + 4 q + e.
BBMPC_TOPK_HD uint32_t topk_first_slot(uint32_t d) { return ((d >> 2) & 3u) * 256u + ((d >> 4) << 2) + (d & 3u); }

// offset keys <= this are winners once the boundary bucket is taken whole (T, top as left by the last pass)
BBMPC_TOPK_HD uint32_t topk_winner_limit(uint32_t span, uint32_t T, int top) {
    const uint32_t hi = top >= 32 ? 0xFFFFFFFFu : (T | ((1u << top) - 1u));
    return hi < span ? hi : span;
}

// ---- the arithmetic of the all-wave route (topk.hpp, block_topk_wave_select): every wave scans the first histogram.
// Host-compilable like everything above (tests/topk_wave_list_check.cpp).
struct TopkQuad {
    uint32_t x, y, z, w;
};
struct TopkPick {
    uint32_t sub;      // which of the lane's 16 consecutive bins holds the k-th key: 4 q + e
    uint32_t wanted;   // how many keys of that bin are still wanted
    uint32_t cnt;      // how many keys it holds
};
// The lane whose 16 bins (four quads c0..c3, `excl` keys in front of them) hold the `remaining`-th key picks the bin with
// a two-level compare and select, operation for operation what topk_scan_first does in wave 0.
BBMPC_TOPK_HD TopkPick topk_pick16(TopkQuad c0, TopkQuad c1, TopkQuad c2, TopkQuad c3, uint32_t excl, uint32_t remaining) {
    const uint32_t s0 = c0.x + c0.y + c0.z + c0.w, s1 = c1.x + c1.y + c1.z + c1.w, s2 = c2.x + c2.y + c2.z + c2.w;
    const uint32_t p1 = excl + s0, p2 = p1 + s1, p3 = p2 + s2;          // keys in front of quads 1, 2, 3
    const bool g1 = remaining > p1, g2 = remaining > p2, g3 = remaining > p3;
    const uint32_t q = (uint32_t)g1 + (uint32_t)g2 + (uint32_t)g3;
    const uint32_t pq = g3 ? p3 : (g2 ? p2 : (g1 ? p1 : excl));
    const uint32_t x = g3 ? c3.x : (g2 ? c2.x : (g1 ? c1.x : c0.x));
    const uint32_t y = g3 ? c3.y : (g2 ? c2.y : (g1 ? c1.y : c0.y));
    const uint32_t z = g3 ? c3.z : (g2 ? c2.z : (g1 ? c1.z : c0.z));
    const uint32_t w = g3 ? c3.w : (g2 ? c2.w : (g1 ? c1.w : c0.w));
    const uint32_t e1 = pq + x, e2 = e1 + y, e3 = e2 + z;               // keys in front of elements 1, 2, 3
    const bool h1 = remaining > e1, h2 = remaining > e2, h3 = remaining > e3;
    const uint32_t e = (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;
    const uint32_t cum = h3 ? e3 : (h2 ? e2 : (h1 ? e1 : pq));
    const uint32_t cnt = h3 ? w : (h2 ? z : (h1 ? y : x));
    return TopkPick{4u * q + e, remaining - cum, cnt};
}

// The all-wave route goes on only when the first pass took the whole boundary bucket in: every key of it is a winner, no
// tie has to be counted and the undecided low bits do not matter (topk_winner_limit covers them).
BBMPC_TOPK_HD bool topk_whole_bucket_in(uint32_t wanted, uint32_t cnt) { return wanted == cnt; }

}  // namespace bbmpc
