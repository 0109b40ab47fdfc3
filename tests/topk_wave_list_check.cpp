// Stand-alone check of the all-wave route's arithmetic in blackbox_mpc_amd/csrc/topk_digits.hpp (plain C++, own main; run
// by tests/test_topk_wave_list_cpu.py).
//
// csrc/topk.hpp's block_topk_wave_select is restated serially from the header -- the key range as the workgroup forms it,
// the first pass's histogram in its LDS layout (topk_first_slot), the scan as a wave does it (lane l sums its 16 bins, an
// exclusive prefix over the lanes, topk_pick16 in the one lane that holds the k-th key), the "whole bucket in" predicate
// and the list of the threads whose offset key is within the winner limit -- and compared with
//   * the selection as it was before (the multi-pass loop, restated below as tests/topk_digits_check.cpp restates it, and
//     the index-ordered list with its exact tie rule), and
//   * a plain stable sort.
// Asserted for every population: the route is taken exactly when the old selection reports ONE pass with
// eq_total == remaining; its list then equals the old one element for element (and the sort's winners); every case it
// declines is one the old code resolves to the sort's winners.
// Populations (N = 1 .. 512, k in {1, 2, 16, 17, 50, 64} with k <= N): random normal, straddling a binade (-128 +- 0.5),
// all equal, -1e6 mixed in, and k - 1 / k / k + 1 copies of the boundary value.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../blackbox_mpc_amd/csrc/topk_digits.hpp"

using namespace bbmpc;

static int g_fail = 0;
static long g_taken = 0, g_declined = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++g_fail < 20) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// ---- the key range of block_topk_prepass: nthr threads (a multiple of 64), thread t holds elements t, t + nthr, ...
static void key_range(const std::vector<float>& v, int k, int nthr, uint32_t& kmin, uint32_t& bound) {
    const int N = (int)v.size();
    std::vector<uint32_t> k1(nthr, 0xFFFFFFFFu), kmx(nthr, 0u);
    for (int n = 0; n < N; ++n) {
        const uint32_t key = reward_key(v[n]);
        k1[n % nthr] = std::min(k1[n % nthr], key);
        kmx[n % nthr] = std::max(kmx[n % nthr], key);
    }
    const int first_round = std::min(N, nthr);
    const int rows_ok = first_round >= 2 ? std::min(nthr >> 4, ((first_round - 2) >> 4) + 1) : 0;
    const bool bound_ok = 2 * rows_ok >= k;
    kmin = 0xFFFFFFFFu;
    bound = 0u;
    for (int row = 0; row < nthr / 16; ++row) {
        uint32_t a = 0xFFFFFFFFu, b = 0xFFFFFFFFu, mx = 0u;
        for (int l = 16 * row; l < 16 * row + 16; ++l) {
            if (k1[l] < a) { b = a; a = k1[l]; } else if (k1[l] < b) b = k1[l];
            mx = std::max(mx, kmx[l]);
        }
        kmin = std::min(kmin, a);
        if (!bound_ok) bound = std::max(bound, mx);
        else if (row < rows_ok) bound = std::max(bound, b);
    }
}

struct Sel {
    uint32_t kmin = 0, T = 0, lim = 0, remaining = 0, eq_total = 0;
    int passes = 0;
};

// ---- the selection as it was: the loop of block_topk_select
static Sel select_old(const std::vector<float>& v, int k, int nthr) {
    const int N = (int)v.size();
    uint32_t kmin, bound;
    key_range(v, k, nthr, kmin, bound);
    const TopkRange rg = topk_range(kmin, bound);
    Sel s;
    s.kmin = kmin;
    int top = rg.top, pass = 0;
    uint32_t T = 0, remaining = (uint32_t)k, eq_total = (uint32_t)N;
    while (top > 0) {
        const int width = topk_pass_width(pass, top), shift = topk_pass_shift(pass, top);
        std::vector<uint32_t> h((size_t)1 << width, 0u);
        for (int n = 0; n < N; ++n) {
            const uint32_t kp = topk_offset_key(v[n], kmin);
            if (topk_takes_part(kp, rg.span, T, top)) h[topk_digit(kp, pass, top)] += 1;
        }
        uint32_t cum = 0, b = 0;
        while (cum + h[b] < remaining) { cum += h[b]; ++b; if (b >= h.size()) { CHECK(false, "ran off the histogram"); return s; } }
        T |= b << shift;
        remaining -= cum;
        eq_total = h[b];
        top = shift;
        ++pass;
        if (eq_total == remaining) break;
    }
    if (pass == 0) eq_total = remaining + 1u;
    s.T = T; s.lim = topk_winner_limit(rg.span, T, top); s.remaining = remaining; s.eq_total = eq_total; s.passes = pass;
    return s;
}

// the index-ordered list of block_topk_finish_indexed (topk_is_winner for every element)
static std::vector<int> list_old(const std::vector<float>& v, const Sel& s) {
    std::vector<int> out;
    uint32_t ties_ahead = 0;
    for (int n = 0; n < (int)v.size(); ++n) {
        const uint32_t kp = topk_offset_key(v[n], s.kmin);
        bool in;
        if (s.eq_total == s.remaining) in = kp <= s.lim;
        else if (kp < s.T) in = true;
        else if (kp != s.T) in = false;
        else { in = ties_ahead < s.remaining; ++ties_ahead; }
        if (in) out.push_back(n);
    }
    return out;
}

// ---- the all-wave route, as ONE wave runs it (every wave runs the same).  Returns false when it declines.
static bool select_wave(const std::vector<float>& v, int k, int nthr, std::vector<int>& list) {
    const int N = (int)v.size();
    uint32_t kmin, bound;
    key_range(v, k, nthr, kmin, bound);
    const TopkRange rg = topk_range(kmin, bound);
    if (rg.top == 0) return false;                                   // span == 0: today's tie path
    const int shift = topk_pass_shift(0, rg.top);
    std::vector<uint32_t> lds(TOPK_BINS1, 0u);                       // the first histogram's LDS words
    for (int n = 0; n < N; ++n) {
        const uint32_t kp = topk_offset_key(v[n], kmin);
        if (topk_takes_part(kp, rg.span, 0u, rg.top)) lds[topk_first_slot(topk_digit(kp, 0, rg.top))] += 1;
    }
    // lane l reads vectors l, 64 + l, 128 + l, 192 + l
    TopkQuad c[64][4];
    uint32_t s[64], incl[64];
    for (int l = 0; l < 64; ++l) {
        s[l] = 0;
        for (int q = 0; q < 4; ++q) {
            const uint32_t* w = &lds[4 * (64 * q + l)];
            c[l][q] = TopkQuad{w[0], w[1], w[2], w[3]};
            s[l] += w[0] + w[1] + w[2] + w[3];
        }
        incl[l] = s[l] + (l ? incl[l - 1] : 0u);
    }
    const uint32_t remaining = (uint32_t)k;
    int holder = -1, holders = 0;
    for (int l = 0; l < 64; ++l)
        if (incl[l] - s[l] < remaining && remaining <= incl[l]) { if (holder < 0) holder = l; ++holders; }
    CHECK(holders == 1, "N %d k %d: %d lanes hold the k-th key", N, k, holders);
    if (holders != 1) return false;
    const TopkPick pk = topk_pick16(c[holder][0], c[holder][1], c[holder][2], c[holder][3], incl[holder] - s[holder], remaining);
    CHECK(pk.sub < 16u, "sub-bin %u", pk.sub);
    const uint32_t bucket = 16u * (uint32_t)holder + pk.sub;
    if (!topk_whole_bucket_in(pk.wanted, pk.cnt)) return false;      // ties at the boundary, or a second pass
    const uint32_t T = bucket << shift;
    const uint32_t lim = topk_winner_limit(rg.span, T, shift);
    // the list: every thread tests the offset key it holds, ascending index order
    list.clear();
    for (int n = 0; n < N; ++n)
        if (topk_offset_key(v[n], kmin) <= lim) list.push_back(n);
    CHECK((int)list.size() == k, "N %d k %d: %zu winners listed", N, k, list.size());
    return true;
}

static bool better(float a, float b) { return a > b; }

static void check_population(const std::vector<float>& v, int k, const char* what) {
    const int N = (int)v.size();
    const int nthr = std::max(64, ((std::max(N, k) + 63) / 64) * 64);            // one element per thread
    const Sel old = select_old(v, k, nthr);
    const std::vector<int> lo = list_old(v, old);
    std::vector<int> ref(N);
    for (int n = 0; n < N; ++n) ref[n] = n;
    std::stable_sort(ref.begin(), ref.end(), [&](int a, int b) { return better(v[a], v[b]); });
    ref.resize(k);
    std::sort(ref.begin(), ref.end());
    CHECK(lo == ref, "%s N %d k %d: the old list is not the sort's", what, N, k);         // every declined case is handled
    std::vector<int> lw;
    const bool took = select_wave(v, k, nthr, lw);
    const bool want = old.passes == 1 && old.eq_total == old.remaining;
    CHECK(took == want, "%s N %d k %d: route taken %d, old selection: %d passes, eq_total %u remaining %u", what, N, k, (int)took,
          old.passes, old.eq_total, old.remaining);
    if (took) {
        ++g_taken;
        CHECK(lw == lo, "%s N %d k %d: the all-wave list differs from the old one", what, N, k);
        CHECK(lw == ref, "%s N %d k %d: the all-wave list is not the sort's", what, N, k);
    } else {
        ++g_declined;
    }
}

struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t u32() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    double uni() { return (u32() + 0.5) / 4294967296.0; }
    float normal() { return (float)(std::sqrt(-2.0 * std::log(uni())) * std::cos(6.283185307179586 * uni())); }
};

static const char* kinds[] = {"normal", "binade", "all equal", "-1e6 mixed", "k-1 copies", "k copies", "k+1 copies"};

static std::vector<float> population(int kind, int N, int k, Rng& r) {
    std::vector<float> v(N);
    for (int n = 0; n < N; ++n) {
        switch (kind) {
            case 1: v[n] = -128.0f + (float)(r.uni() - 0.5); break;              // straddles the binade at -128
            case 2: v[n] = -3.25f; break;
            case 3: v[n] = (r.u32() % 3 == 0) ? -1.0e6f : -100.0f + 30.0f * r.normal(); break;
            default: v[n] = -100.0f + 30.0f * r.normal(); break;
        }
    }
    if (kind >= 4) {        // copies of the boundary (k-th best) value: k - 1, k or k + 1 of them, as far as N allows
        std::vector<float> s(v);
        std::sort(s.begin(), s.end(), better);
        const float val = s[k - 1];
        const int copies = std::min(N, k + kind - 5);
        for (int i = 0; i < copies; ++i) v[(size_t)((uint64_t)i * 2654435761u % (uint32_t)N)] = val;
    }
    return v;
}

int main() {
    Rng r(20240607);
    const int ks[6] = {1, 2, 16, 17, 50, 64};
    for (int N = 1; N <= 512; ++N)
        for (int ki = 0; ki < 6; ++ki) {
            const int k = ks[ki];
            if (k > N) continue;
            for (int kind = 0; kind < 7; ++kind) check_population(population(kind, N, k, r), k, kinds[kind]);
        }
    // the binade population of the pass-count check in tests/topk_digits_check.cpp: one pass, the route is taken
    {
        std::vector<float> v(500);
        for (int n = 0; n < 500; ++n) v[n] = -127.5f - (float)n / 499.0f;
        std::vector<int> lw;
        CHECK(select_wave(v, 50, 512, lw), "evenly spaced over -128 +- 0.5: the route declined");
        check_population(v, 50, "evenly spaced");
    }
    CHECK(g_taken > 1000 && g_declined > 1000, "route taken %ld times, declined %ld times: both must be exercised", g_taken, g_declined);
    printf("route taken %ld times, declined %ld times\n", g_taken, g_declined);
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("all checks held\n");
    return 0;
}
