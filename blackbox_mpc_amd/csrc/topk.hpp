// Exact sorted top-k of a workgroup's LDS-resident rewards: tf.nn.top_k(sorted=True) semantics
// (cem.py:97-99) -- larger first, ties -> lower index first.
//
// MSD radix select on order-preserving 32-bit keys, taken as OFFSETS from the smallest key (topk_digits.hpp holds the
// arithmetic, for the kernels and for a CPU program alike): with B an upper bound of the k-th smallest key, only keys
// within span = B - kmin take part, the first pass takes the top TOPK_W1 = 10 bits of the span (1024 bins), later
// passes 8 bits each -- <= 4 passes, each one LDS histogram (ds_add_u32, a few dozen per pass: keys above the bound
// issue none) + one scan by a single wave, i.e. O(N) work per pass instead of the O(N^2) comparison count of ranking by
// counting.  A pass is two barriers; most selections of a CEM population end after the first (a digit taken below the
// highest bit in which kmin and B DIFFER left two or three bins to a population that straddles a binade, and a second
// pass to five selections in six: profiles/cem_select_offset_digits.md).  That pins the k-th key exactly; the <= k
// winners are then listed in index order, or compacted and ranked among themselves (k^2 comparisons on 64-bit
// (key,index) words).
//
// LDS (TOPK_HIST_WORDS): second histogram [256] | control words [16] | first histogram [1024].  Pass 0 uses the first
// histogram (bins at topk_first_slot(), so that wave 0's four 16-byte reads per lane are conflict free), pass 1 the
// second, pass 2 the first 256 words of the first, ...; the array of pass p + 1 is zeroed while pass p is scanned.
// The per-wave (kmin, bound) slots live in words [0, 32) of the second histogram.
// WIDE = false (the CMA-ES kernels): 8 bits in the first pass as well, TOPK_HIST_WORDS_NARROW words, the LDS these
// kernels had before the wide pass -- their population limit is set by the words beside the rewards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topk_digits.hpp"

namespace bbmpc {

// inclusive prefix sum over the 64 lanes: DPP row_shr scan inside each 16-lane row, row totals via readlane
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
    int x = (int)v;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    const int t0 = __builtin_amdgcn_readlane(x, 15), t1 = __builtin_amdgcn_readlane(x, 31),
              t2 = __builtin_amdgcn_readlane(x, 47);
    const int row = lane >> 4;
    x += (row >= 1 ? t0 : 0) + (row >= 2 ? t1 : 0) + (row >= 3 ? t2 : 0);
    return (uint32_t)x;
}

// vals[N] in LDS (left untouched); eidx[k] out; hist[TOPK_HIST_WORDS] and ekeys[k] are LDS scratch.
// All threads of the workgroup must call (k <= nthr); ends with a barrier (eidx visible to everyone).
// Barrier budget: 1 (key range) + 2 per radix pass (usually 1 pass) + 1 (compaction) + 2 (ranking); the index-ordered
// finish: 1 per round of nthr elements + 1.  The 512-thread CEM control step in its common case (one element per thread,
// k <= 64, a first pass that takes the whole boundary bucket in: block_topk_wave_select): 1 (key range) + 1 (histogram)
// + 2 (the list) -- every wave scans for itself, the scan's barrier is gone (profiles/cem_wave_select.md).
#ifdef BBMPC_KERNEL_DBG
__shared__ long long g_topk_dbg[16];
#define TOPK_DBG(i) do { if (tid == 0) g_topk_dbg[(i)] = (long long)wall_clock64(); } while (0)
#else
#define TOPK_DBG(i) do {} while (0)
#endif

// Keys are OFFSET keys throughout (reward_key(r) - kmin): T, lim and the key halves of ekeys[] (the order is the same
// as the real keys').
struct TopkSel {
    uint32_t kmin;       // smallest key of the population
    uint32_t T;          // decided high bits of the k-th offset key
    uint32_t lim;        // eq_total == remaining: offset keys <= lim are the winners (topk_winner_limit)
    uint32_t remaining;  // how many keys of the boundary bucket are winners
    uint32_t eq_total;   // how many keys the boundary bucket holds; != remaining only with no low bit left undecided
    int passes;          // radix passes the selection took (0: min == bound)
};

// First part of the selection, up to (not including) its first barrier: every thread reads only the elements
// n = tid, tid + nthr, ... -- a caller whose threads have just WRITTEN exactly those elements (the persistent kernel's
// rollout) runs it in front of the barrier it needs anyway and then calls block_topk_select(..., prepass_done = true).
// SPLIT (the all-wave route, block_topk_wave_select): the per-wave slots go to smin[wave] / sbound[wave], words of the
// caller's outside hist[], and the second histogram and the compaction cursor are zeroed HERE, half a word per thread
// at 512 threads -- that route has no scan phase in which idle waves could zero them.  INVARIANT: with SPLIT nothing in
// hist[] is read between this zeroing and the barrier behind it, and the slots, read behind that barrier, are not in it.
template <bool WIDE = true, bool SPLIT = false>
__device__ __forceinline__ void block_topk_prepass(const float* vals, int N, int k, uint32_t* hist, int tid, int nthr,
                                                   uint32_t* smin = nullptr, uint32_t* sbound = nullptr) {
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t* hist2 = hist + TOPK_HIST2_OFF;     // second histogram; its first 32 words carry the per-wave slots first
    // ---- key range: digits are taken from the top of span = B - min, B an UPPER BOUND of the k-th smallest key.
    // Rewards of one population mostly share sign + exponent, so a fixed top-8-bit digit would send a whole wave's
    // ds_add_u32 to one or two bins (serialised); and the worst rewards are far outliers, so [min, max] would still
    // squeeze everything that matters into a few bins.  Bound: every 16-lane row contributes its two smallest keys
    // (distinct elements); if that makes >= k elements, the largest of them is >= the k-th smallest overall.  Keys
    // above B never enter a histogram.
    uint32_t k1 = 0xFFFFFFFFu, kmaxl = 0u;           // this lane's smallest key (one element per lane) / largest
    for (int n = tid; n < N; n += nthr) {
        const uint32_t key = reward_key(vals[n]);
        k1 = min(k1, key);
        kmaxl = max(kmaxl, key);
    }
    uint32_t k2 = 0xFFFFFFFFu;                       // (k1 <= k2): two smallest of the lanes merged so far
    // mirror butterfly inside the 16-lane row: every step merges DISJOINT lane sets, so (min, second min) stay exact
#define BB_ROW_MIN2(ctrl) do {                                                                              \
        const uint32_t o1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k1, ctrl, 0xf, 0xf, false);             \
        const uint32_t o2 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)k2, ctrl, 0xf, 0xf, false);             \
        const uint32_t hi1 = max(k1, o1);                                                                         \
        k1 = min(k1, o1);                                                                                         \
        k2 = min(hi1, min(k2, o2));                                                                               \
    } while (0)
    BB_ROW_MIN2(0xB1); BB_ROW_MIN2(0x4E); BB_ROW_MIN2(0x141); BB_ROW_MIN2(0x140);
#undef BB_ROW_MIN2
#define BB_ROW_U32(op, v, ctrl) v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xf, 0xf, false))
    BB_ROW_U32(max, kmaxl, 0xB1); BB_ROW_U32(max, kmaxl, 0x4E); BB_ROW_U32(max, kmaxl, 0x141); BB_ROW_U32(max, kmaxl, 0x140);
#undef BB_ROW_U32
    // rows that hold fewer than two elements do not take part in the bound
    const int first_round = min(N, nthr);            // lanes tid < first_round hold an element
    const int rows_ok = first_round >= 2 ? min(nthr >> 4, ((first_round - 2) >> 4) + 1) : 0;
    const bool bound_ok = 2 * rows_ok >= k;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wave * 4 + r;
        kmin = min(kmin, (uint32_t)__builtin_amdgcn_readlane((int)k1, 16 * r));
        const uint32_t b = bound_ok ? (uint32_t)__builtin_amdgcn_readlane((int)k2, 16 * r)
                                    : (uint32_t)__builtin_amdgcn_readlane((int)kmaxl, 16 * r);
        if (!bound_ok || row < rows_ok) kmax = max(kmax, b);
    }
    // per-wave slots instead of atomics; the min of wave w goes to hist2[w], the bound to hist2[16+w]: the first pass
    // does not use that array, and it is zeroed for the second one behind the barrier all slots are read in front of
    if constexpr (SPLIT) {
        if (lane == 0) { smin[wave] = kmin; sbound[wave] = kmax; }
        uint2* hz2 = reinterpret_cast<uint2*>(hist2);
        for (int i = tid; i < TOPK_BINSN / 2; i += nthr) hz2[i] = make_uint2(0u, 0u);
        if (tid == 0) hist[TOPK_CTRL_OFF + 3] = 0u;
    } else {
        if (lane == 0) { hist2[wave] = kmin; hist2[16 + wave] = kmax; }
    }
    // the first pass histograms into the first histogram's 1024 words: two words per thread at 512 threads
    uint2* hz = reinterpret_cast<uint2*>(hist + TOPK_HIST1_OFF);
    for (int i = tid; i < (WIDE ? TOPK_BINS1 : TOPK_BINSN) / 2; i += nthr) hz[i] = make_uint2(0u, 0u);
}

// wave 0's part of a pass over the FIRST histogram (1024 bins at topk_first_slot()): lane l holds the 16 consecutive bins
// 16 l .. 16 l + 15 in four vectors; after the wave scan has found the lane, the bin is found among its 16 with a
// two-level compare and select (the quad, then the element) -- no serial search, no indexed register array.
__device__ __forceinline__ void topk_scan_first(const uint32_t* h, uint32_t* ctrl, uint32_t remaining, int lane) {
    const uint4* hv = reinterpret_cast<const uint4*>(h);
    const uint4 c0 = hv[lane], c1 = hv[64 + lane], c2 = hv[128 + lane], c3 = hv[192 + lane];
    const uint32_t s0 = c0.x + c0.y + c0.z + c0.w, s1 = c1.x + c1.y + c1.z + c1.w;
    const uint32_t s2 = c2.x + c2.y + c2.z + c2.w, s3 = c3.x + c3.y + c3.z + c3.w;
    const uint32_t s = (s0 + s1) + (s2 + s3);
    const uint32_t incl = wave_incl_scan(s, lane);
    const uint32_t excl = incl - s;
    if (excl < remaining && remaining <= incl) {            // exactly one lane
        const uint32_t p1 = excl + s0, p2 = p1 + s1, p3 = p2 + s2;       // keys in front of quads 1, 2, 3
        const bool g1 = remaining > p1, g2 = remaining > p2, g3 = remaining > p3;       // (g3 => g2 => g1)
        const uint32_t q = (uint32_t)g1 + (uint32_t)g2 + (uint32_t)g3;
        const uint32_t pq = g3 ? p3 : (g2 ? p2 : (g1 ? p1 : excl));
        const uint32_t x = g3 ? c3.x : (g2 ? c2.x : (g1 ? c1.x : c0.x));
        const uint32_t y = g3 ? c3.y : (g2 ? c2.y : (g1 ? c1.y : c0.y));
        const uint32_t z = g3 ? c3.z : (g2 ? c2.z : (g1 ? c1.z : c0.z));
        const uint32_t w = g3 ? c3.w : (g2 ? c2.w : (g1 ? c1.w : c0.w));
        const uint32_t e1 = pq + x, e2 = e1 + y, e3 = e2 + z;            // keys in front of elements 1, 2, 3
        const bool h1 = remaining > e1, h2 = remaining > e2, h3 = remaining > e3;
        const uint32_t e = (uint32_t)h1 + (uint32_t)h2 + (uint32_t)h3;
        const uint32_t cum = h3 ? e3 : (h2 ? e2 : (h1 ? e1 : pq));
        const uint32_t cnt = h3 ? w : (h2 ? z : (h1 ? y : x));
        ctrl[0] = 16u * (uint32_t)lane + 4u * q + e;
        ctrl[1] = remaining - cum;     // how many keys of this bucket are still wanted
        ctrl[2] = cnt;                 // how many keys the bucket holds
        ctrl[3] = 0;                   // compaction cursor
    }
}

// The radix passes of a selection from pass `pass` on, with `top` low bits of the k-th offset key undecided, T its decided
// high bits, `remaining` keys still wanted from the bucket T names and eq_total keys in it.  block_topk_select enters at
// pass 0; the all-wave route (block_topk_wave_select) has run the first pass itself and enters at pass 1 when that did not
// take the whole boundary bucket in -- with the second histogram and ctrl[3] zeroed, as the idle waves of pass 0 leave them.
// Ends with a barrier whenever it ran a pass or pass == 0; ctrl[3] (compaction cursor) is 0.
template <bool WIDE = true>
__device__ __forceinline__ TopkSel topk_select_passes(const float* vals, int N, uint32_t* hist, int tid, int nthr, uint32_t kmin,
                                                      uint32_t span, int top, uint32_t T, uint32_t remaining, uint32_t eq_total,
                                                      int pass) {
    const int lane = tid & 63;
    uint32_t* ctrl = hist + TOPK_CTRL_OFF;       // [0] bucket [1] wanted [2] bucket size [3] compaction cursor
    uint32_t* hist2 = hist + TOPK_HIST2_OFF;
    uint32_t* hist1 = hist + TOPK_HIST1_OFF;
    constexpr int W1 = WIDE ? TOPK_W1 : TOPK_WN;
    // The first pass uses the 1024-bin histogram (zeroed before the barrier; the slots read above are in hist2), the
    // second hist2, later ones alternate between the first 256 words of hist1 and hist2; the array for pass p+1 is zeroed
    // by the idle waves while wave 0 scans pass p.
    while (top > 0) {
        uint32_t* h = (pass & 1) ? hist2 : hist1;
        uint32_t* hn = (pass & 1) ? hist1 : hist2;
        const int shift = topk_pass_shift(pass, top, W1);
        for (int n = tid; n < N; n += nthr) {
            const uint32_t kp = topk_offset_key(vals[n], kmin);
            if (topk_takes_part(kp, span, T, top)) {
                const uint32_t d = topk_digit(kp, pass, top, W1);
                const uint32_t slot = (WIDE && pass == 0) ? topk_first_slot(d) : d;
#ifdef BBMPC_EXP_NOATOMIC
                h[slot] = 1u;
#else
                atomicAdd(&h[slot], 1u);
#endif
            }
        }
        __syncthreads();
        TOPK_DBG(2 + 2 * pass);
        if (tid < 64) {
            if (WIDE && pass == 0) {
                topk_scan_first(h, ctrl, remaining, lane);
            } else {
                const uint4 c = *reinterpret_cast<const uint4*>(h + 4 * lane);
                const uint32_t s = c.x + c.y + c.z + c.w;
                const uint32_t incl = wave_incl_scan(s, lane);
                const uint32_t excl = incl - s;
                if (excl < remaining && remaining <= incl) {        // exactly one lane
                    uint32_t cum = excl, b = 4 * lane, cnt = c.x;
                    if (cum + c.x < remaining) { cum += c.x; b += 1; cnt = c.y;
                        if (cum + c.y < remaining) { cum += c.y; b += 1; cnt = c.z;
                            if (cum + c.z < remaining) { cum += c.z; b += 1; cnt = c.w; } } }
                    ctrl[0] = b;
                    ctrl[1] = remaining - cum;     // how many keys of this bucket are still wanted
                    ctrl[2] = cnt;                 // how many keys the bucket holds
                    ctrl[3] = 0;                   // compaction cursor
                }
            }
        } else {
            for (int i = tid - 64; i < TOPK_BINSN; i += nthr - 64) hn[i] = 0;
        }
        if (nthr == 64)
            for (int i = tid; i < TOPK_BINSN; i += 64) hn[i] = 0;
        __syncthreads();
        TOPK_DBG(3 + 2 * pass);
        // (every lane reads the same words: scalar registers)
        T |= (uint32_t)__builtin_amdgcn_readfirstlane((int)ctrl[0]) << shift;
        remaining = (uint32_t)__builtin_amdgcn_readfirstlane((int)ctrl[1]);
        eq_total = (uint32_t)__builtin_amdgcn_readfirstlane((int)ctrl[2]);
        top = shift;
        ++pass;
        if (eq_total == remaining) break;      // every key of the boundary bucket is a winner: the undecided
    }                                          // low bits no longer matter
    if (pass == 0) {                           // min == bound: at least k keys tie for best; no pass ran, so the
        if (tid == 0) ctrl[3] = 0;             // bucket size is unknown and nobody reset the cursor: force the
        __syncthreads();                       // exact tie path (lowest indices win)
        eq_total = remaining + 1u;
    }
    return TopkSel{kmin, T, topk_winner_limit(span, T, top), remaining, eq_total, pass};
}

// Selection only: pins the boundary bucket of the k-th key.  Ends with a barrier; ctrl[3] (compaction cursor) is 0.
template <bool WIDE = true>
__device__ __forceinline__ TopkSel block_topk_select(const float* vals, int N, int k, uint32_t* hist, int tid, int nthr,
                                                     bool prepass_done = false, const uint32_t* smin = nullptr,
                                                     const uint32_t* sbound = nullptr) {      // (slots of a SPLIT prepass)
    const int lane = tid & 63, nw = nthr >> 6;
    TOPK_DBG(0);
    uint32_t* hist2 = hist + TOPK_HIST2_OFF;     // second histogram; its first 32 words carry the per-wave slots first
    if (!prepass_done) {
        block_topk_prepass<WIDE>(vals, N, k, hist, tid, nthr);
        __syncthreads();
    }
    uint32_t kmin, kmax;
    TOPK_DBG(1);
    // combine the (<= 16) per-wave slots with ONE LDS round trip: lane w fetches wave w's pair, then a 16-lane DPP
    // reduction (a serial loop over the slots costs one LDS latency per wave)
    kmin = 0xFFFFFFFFu; kmax = 0u;
    if (lane < nw) { kmin = smin ? smin[lane] : hist2[lane]; kmax = sbound ? sbound[lane] : hist2[16 + lane]; }
#define BB_ROW_U32(op, v, ctrl) v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xf, 0xf, false))
    BB_ROW_U32(min, kmin, 0xB1); BB_ROW_U32(min, kmin, 0x4E); BB_ROW_U32(min, kmin, 0x141); BB_ROW_U32(min, kmin, 0x140);
    BB_ROW_U32(max, kmax, 0xB1); BB_ROW_U32(max, kmax, 0x4E); BB_ROW_U32(max, kmax, 0x141); BB_ROW_U32(max, kmax, 0x140);
#undef BB_ROW_U32
    kmin = (uint32_t)__builtin_amdgcn_readlane((int)kmin, 0);
    kmax = (uint32_t)__builtin_amdgcn_readlane((int)kmax, 0);
    const TopkRange rg = topk_range(kmin, kmax);
    // top: the number of low bits of the k-th OFFSET key still undecided; T = 0: its decided high bits;
    // eq_total = N: span == 0 means at least k keys equal the smallest
    return topk_select_passes<WIDE>(vals, N, hist, tid, nthr, kmin, rg.span, rg.top, 0u, (uint32_t)k, (uint32_t)N, 0);
}

// Winner test for element n given the selection (exact ties at the boundary: lowest indices win)
__device__ __forceinline__ bool topk_is_winner(const float* vals, int n, const TopkSel& s) {
    const uint32_t kp = topk_offset_key(vals[n], s.kmin);
    if (s.eq_total == s.remaining) return kp <= s.lim;           // the whole boundary bucket is in
    if (kp < s.T) return true;                                   // no low bit is undecided here (rare): T is the k-th key
    if (kp != s.T) return false;
    uint32_t before = 0;                                         // count equal keys ahead of n
    for (int m = 0; m < n; ++m) before += (topk_offset_key(vals[m], s.kmin) == s.T) ? 1u : 0u;
    return before < s.remaining;
}

// Finish A: the k winners in ASCENDING INDEX order (a deterministic order that needs no ranking): per-wave
// ballot + mbcnt prefix, wave totals through LDS.  Used where only the elite SET matters (CEM's refit).
// One barrier per round of nthr elements + the closing one.
__device__ __forceinline__ void block_topk_finish_indexed(const float* vals, int N, int k, int* eidx, uint32_t* hist,
                                                          const TopkSel& sel, int tid, int nthr) {
    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    uint32_t* wtot = hist;                                       // [2][16] wave totals, double buffered per round
    uint32_t base = 0;
    int round = 0;
    for (int n0 = 0; n0 < N; n0 += nthr, ++round) {
        const int n = n0 + tid;
        const bool take = (n < N) && topk_is_winner(vals, n, sel);
        const unsigned long long bal = __ballot(take);
        const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        uint32_t* wt = wtot + (round & 1) * 16;
        if (lane == 0) wt[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        TOPK_DBG(8);      // (slots 8 / 9 are a fourth pass's too; the clocked runs never take one)
        // lane w fetches wave w's total (one LDS round trip), 16-lane DPP prefix scan, results through readlane
        int x = (lane < nw) ? (int)wt[lane] : 0;
        x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
        x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
        x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
        x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
        const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane(x, 15);
        const uint32_t incl_w = (uint32_t)__builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(wave));
        const uint32_t off = base + incl_w - (uint32_t)__popcll(bal);
        if (take) eidx[off + pre] = n;
        base += tot;
    }
    __syncthreads();
    TOPK_DBG(9);
}

// ---- The all-wave route of the 512-thread CEM control step (kernels_fused.hpp): behind the histogram's barrier EVERY
// wave scans the first histogram -- what wave 0 handed the others across the scan's barrier (ctrl[]) is a pure function
// of the first histogram, which every wave sees behind the histogram's barrier -- and, when the first pass took the whole
// boundary bucket in, tests the offset key it kept in a register and lists the winners as block_topk_finish_indexed does.
// Barrier budget of that case: 1 (key range; the caller's) + 1 (histogram) + 2 (the list).
// Needs: one element per thread (N <= nthr <= 512), k <= 64, block_topk_prepass<true, true> done and its barrier passed.
// Every case it declines -- span == 0, a first pass that leaves ties or a second pass to do -- runs today's code from
// where it is detected; every wave computes the same scan, so the decision is uniform without communication.
// Returns TOPK_ROUTE_OLD: `sel` is filled as block_topk_select fills it, the caller finishes (block_topk_finish_indexed);
//         TOPK_ROUTE_LIST: eidx[0..k) written in ascending index order, closing barrier passed.
// (Every wave listing all winners into a copy of its own, with no barrier up to the statistics, was built and measured
// 1.6 us per control step SLOWER than this: profiles/cem_wave_select.md.)
constexpr int TOPK_ROUTE_OLD = 0, TOPK_ROUTE_LIST = 1;

struct TopkWavePick {
    uint32_t bucket, wanted, cnt;
};
// topk_scan_first in every wave: the same reads and arithmetic, the pick broadcast from the one lane that holds it
__device__ __forceinline__ TopkWavePick topk_scan_first_all(const uint32_t* h, uint32_t remaining, int lane) {
    const uint4* hv = reinterpret_cast<const uint4*>(h);
    const uint4 c0 = hv[lane], c1 = hv[64 + lane], c2 = hv[128 + lane], c3 = hv[192 + lane];
    const uint32_t s0 = c0.x + c0.y + c0.z + c0.w, s1 = c1.x + c1.y + c1.z + c1.w;
    const uint32_t s2 = c2.x + c2.y + c2.z + c2.w, s3 = c3.x + c3.y + c3.z + c3.w;
    const uint32_t s = (s0 + s1) + (s2 + s3);
    const uint32_t incl = wave_incl_scan(s, lane);
    const uint32_t excl = incl - s;
    const TopkPick pk = topk_pick16(TopkQuad{c0.x, c0.y, c0.z, c0.w}, TopkQuad{c1.x, c1.y, c1.z, c1.w}, TopkQuad{c2.x, c2.y, c2.z, c2.w},
                                    TopkQuad{c3.x, c3.y, c3.z, c3.w}, excl, remaining);
    const unsigned long long holder = __ballot(excl < remaining && remaining <= incl);      // exactly one lane
    const int src = holder ? __builtin_ctzll(holder) : 0;
    TopkWavePick r;
    r.bucket = 16u * (uint32_t)src + (uint32_t)__builtin_amdgcn_readlane((int)pk.sub, src);
    r.wanted = (uint32_t)__builtin_amdgcn_readlane((int)pk.wanted, src);
    r.cnt = (uint32_t)__builtin_amdgcn_readlane((int)pk.cnt, src);
    return r;
}

__device__ __forceinline__ int block_topk_wave_select(const float* vals, int N, int k, int* eidx, uint32_t* hist, const uint32_t* smin,
                                                      const uint32_t* sbound, int tid, int nthr, TopkSel& sel) {
    const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
    uint32_t* hist1 = hist + TOPK_HIST1_OFF;
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
    if (lane < nw) { kmin = smin[lane]; kmax = sbound[lane]; }
#define BB_ROW_U32(op, v, ctrl) v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(v), ctrl, 0xf, 0xf, false))
    BB_ROW_U32(min, kmin, 0xB1); BB_ROW_U32(min, kmin, 0x4E); BB_ROW_U32(min, kmin, 0x141); BB_ROW_U32(min, kmin, 0x140);
    BB_ROW_U32(max, kmax, 0xB1); BB_ROW_U32(max, kmax, 0x4E); BB_ROW_U32(max, kmax, 0x141); BB_ROW_U32(max, kmax, 0x140);
#undef BB_ROW_U32
    kmin = (uint32_t)__builtin_amdgcn_readlane((int)kmin, 0);
    kmax = (uint32_t)__builtin_amdgcn_readlane((int)kmax, 0);
    const TopkRange rg = topk_range(kmin, kmax);
    const uint32_t span = rg.span;
    if (rg.top == 0) {                           // min == bound: the exact tie path, today's code (no pass runs)
        sel = topk_select_passes<true>(vals, N, hist, tid, nthr, kmin, span, 0, 0u, (uint32_t)k, (uint32_t)N, 0);
        return TOPK_ROUTE_OLD;
    }
    // ---- the first pass's histogram; the thread keeps its offset key for the winner test
    const int shift = topk_pass_shift(0, rg.top, TOPK_W1);
    uint32_t kp = 0xFFFFFFFFu;
    if (tid < N) {
        kp = topk_offset_key(vals[tid], kmin);
        if (topk_takes_part(kp, span, 0u, rg.top)) atomicAdd(&hist1[topk_first_slot(topk_digit(kp, 0, rg.top, TOPK_W1))], 1u);
    }
    __syncthreads();
    TOPK_DBG(2);
    const TopkWavePick pk = topk_scan_first_all(hist1, (uint32_t)k, lane);
    const uint32_t T = pk.bucket << shift;
    if (!topk_whole_bucket_in(pk.wanted, pk.cnt)) {      // ties at the boundary or a second pass: today's loop from pass 1
        sel = topk_select_passes<true>(vals, N, hist, tid, nthr, kmin, span, shift, T, pk.wanted, pk.cnt, 1);
        return TOPK_ROUTE_OLD;
    }
    const uint32_t lim = topk_winner_limit(span, T, shift);
    sel = TopkSel{kmin, T, lim, pk.wanted, pk.cnt, 1};
    // block_topk_finish_indexed's one round (N <= nthr) on the key the thread holds
    uint32_t* wt = hist;                                     // [16] wave totals (hist2's first words, as there)
    const bool take = tid < N && kp <= lim;
    const unsigned long long bal = __ballot(take);
    const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (lane == 0) wt[wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    TOPK_DBG(3);
    int x = (lane < nw) ? (int)wt[lane] : 0;
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xf, 0xf, false);   // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xf, 0xf, false);   // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xf, 0xf, false);   // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xf, 0xf, false);   // row_shr:8
    const uint32_t incl_w = (uint32_t)__builtin_amdgcn_readlane(x, __builtin_amdgcn_readfirstlane(wave));
    if (take) eidx[incl_w - (uint32_t)__popcll(bal) + pre] = tid;
    __syncthreads();
    return TOPK_ROUTE_LIST;
}

// Finish B: the k winners sorted (tf.nn.top_k(sorted=True)): atomic compaction + k x k ranking.
__device__ __forceinline__ void block_topk_finish_sorted(const float* vals, int N, int k, int* eidx, uint32_t* hist,
                                                         unsigned long long* ekeys, const TopkSel& sel, int tid, int nthr) {
    uint32_t* ctrl = hist + TOPK_CTRL_OFF;
    const uint32_t T = sel.T, remaining = sel.remaining, eq_total = sel.eq_total, kmin = sel.kmin;
    // ---- compaction of the winners (any order); low bits may be undecided after an early exit: sel.lim covers them
    for (int e = tid; e < k; e += nthr) eidx[e] = 0;             // rank counters for the next phase
    if (eq_total == remaining) {                                 // the whole boundary bucket is in (the usual case)
        for (int n = tid; n < N; n += nthr) {
            const uint32_t key = topk_offset_key(vals[n], kmin);
            if (key <= sel.lim) {
                const uint32_t slot = atomicAdd(&ctrl[3], 1u);
                ekeys[slot] = ((unsigned long long)key << 32) | (uint32_t)n;
            }
        }
        __syncthreads();
    } else {
        // no low bit undecided here: more keys EQUAL the k-th one than are wanted, the lowest indices win.  The number of equal keys
        // ahead of element n comes from a ballot / prefix count per wave and the waves' totals (one barrier per round of
        // nthr elements) -- counting them one by one per element was 25-30 us when a hundred candidates tie, which is the
        // steady state of CMA-ES on the pendulum: its step size is never reset (cma_es.py:215-227 restores m and sigma at
        // an episode's start only), after 40 control steps sigma is 2e-5 and the 500 rewards take ten distinct values
        // (profiles/NOTES_r4.md)
        const int lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
        uint32_t* wtot = hist;                                   // [2][16] wave totals, double buffered per round
        uint32_t base = 0;
        int round = 0;
        for (int n0 = 0; n0 < N; n0 += nthr, ++round) {
            const int n = n0 + tid;
            const uint32_t key = n < N ? topk_offset_key(vals[n], kmin) : 0xFFFFFFFFu;
            const bool tie = n < N && key == T;
            const unsigned long long bal = __ballot(tie);
            const uint32_t pre = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
            uint32_t* wt = wtot + (round & 1) * 16;
            if (lane == 0) wt[wave] = (uint32_t)__popcll(bal);
            __syncthreads();
            uint32_t ahead = base, tot = 0;
            for (int w = 0; w < nw; ++w) { const uint32_t c = wt[w]; ahead += (w < wave) ? c : 0u; tot += c; }
            const bool take = n < N && (key < T || (tie && ahead + pre < remaining));
            if (take) {
                const uint32_t slot = atomicAdd(&ctrl[3], 1u);
                ekeys[slot] = ((unsigned long long)key << 32) | (uint32_t)n;
            }
            base += tot;
        }
        __syncthreads();
    }
    // ---- rank the k winners among themselves with the whole workgroup: thread (e, chunk) counts how many
    // winners in its chunk precede winner e, partial counts meet in LDS (eidx doubles as the counter array).
    const int kp64 = (k + 63) & ~63;                 // e runs over full waves so chunk ids are wave-uniform
    const int nchunk = max(1, nthr / kp64);
    const int clen = (k + nchunk - 1) / nchunk;
    for (int t = tid; t < kp64 * nchunk; t += nthr) {
        const int e = t % kp64, c = t / kp64;
        if (e < k) {
            const unsigned long long mine = ekeys[e];
            const int o0 = c * clen, o1 = min(k, o0 + clen);
            int cnt = 0;
#pragma unroll 4
            for (int o = o0; o < o1; ++o) cnt += (ekeys[o] < mine) ? 1 : 0;
            if (cnt) atomicAdd((uint32_t*)&eidx[e], (uint32_t)cnt);
        }
    }
    __syncthreads();
    int myrank = -1, myidx = 0;
    if (tid < k) { myrank = eidx[tid]; myidx = (int)(uint32_t)(ekeys[tid] & 0xFFFFFFFFull); }
    __syncthreads();
    if (myrank >= 0) eidx[myrank] = myidx;
    __syncthreads();
}

// vals[N] in LDS (left untouched); eidx[k] out; hist[TOPK_HIST_WORDS] and ekeys[k] are LDS scratch.
// All threads of the workgroup must call (k <= nthr); ends with a barrier (eidx visible to everyone).
// Returns the number of radix passes the selection took.
template <bool WIDE = true>
__device__ __forceinline__ int block_topk_sorted(const float* vals, int N, int k, int* eidx, uint32_t* hist,
                                                 unsigned long long* ekeys, int tid, int nthr) {
    const TopkSel sel = block_topk_select<WIDE>(vals, N, k, hist, tid, nthr);
    block_topk_finish_sorted(vals, N, k, eidx, hist, ekeys, sel, tid, nthr);
    return sel.passes;
}

}  // namespace bbmpc
