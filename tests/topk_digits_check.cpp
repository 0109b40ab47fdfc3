// Stand-alone check of blackbox_mpc_amd/csrc/topk_digits.hpp (plain C++, own main; run by tests/test_topk_digits_cpu.py).
//
// The radix select of csrc/topk.hpp is restated serially -- the key range as the workgroup forms it (per-lane minima, the
// two smallest keys of every 16-lane row, the bound from the rows that hold two elements), then the multi-pass loop with
// the header's offset keys, widths, digits and participation test, the early exit and the exact-tie rule -- and compared
// with a brute-force stable sort:
//   * the winner set (ascending index) and the sorted order (larger reward first, ties to the lower index), for
//     N = 1 .. 1100 and k in {1, 2, 50, 64, N} on eight kinds of input (see kinds[] below);
//   * 500 rewards evenly spaced over -128 +- 0.5, k = 50: exactly one pass; the same population under a restatement of
//     the rule this one replaced (digits below the highest bit in which kmin and the bound differ; kept HERE only): two
//     or more;
//   * span == 0: no pass; no input: more than TOPK_MAX_PASSES passes;
//   * the narrow form (8 bits in the first pass too, what the CMA-ES kernels run) on every seventh N: the same winners.
//
//   topk_digits_check                      runs the checks
//   topk_digits_check --passes FILE        FILE: int32 M, N, k, nthr, then M x N float32 rewards.  Prints per population
//                                          "passes excess old_passes old_excess": the passes of this rule and of the old
//                                          one, and how many keys too many the first pass's boundary bucket held.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../blackbox_mpc_amd/csrc/topk_digits.hpp"

using namespace bbmpc;

static int g_fail = 0;
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
        uint32_t a = 0xFFFFFFFFu, b = 0xFFFFFFFFu, mx = 0u;          // the row's two smallest lane minima, its largest key
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
    long excess = 0;          // keys too many in the first pass's boundary bucket
};

// ---- the loop of block_topk_select, from the header
static Sel select_offset(const std::vector<float>& v, int k, int nthr, int w1 = TOPK_W1) {
    const int N = (int)v.size();
    uint32_t kmin, bound;
    key_range(v, k, nthr, kmin, bound);
    const TopkRange rg = topk_range(kmin, bound);
    Sel s;
    s.kmin = kmin;
    int top = rg.top;
    uint32_t T = 0, remaining = (uint32_t)k, eq_total = (uint32_t)N;
    int pass = 0;
    while (top > 0) {
        const int width = topk_pass_width(pass, top, w1), shift = topk_pass_shift(pass, top, w1);
        std::vector<uint32_t> h((size_t)1 << width, 0u);
        std::vector<uint32_t> slots(TOPK_BINS1, 0u);                  // the first pass's LDS words: a permutation of the bins
        for (int n = 0; n < N; ++n) {
            const uint32_t kp = topk_offset_key(v[n], kmin);
            if (!topk_takes_part(kp, rg.span, T, top)) continue;
            const uint32_t d = topk_digit(kp, pass, top, w1);
            CHECK(d < h.size(), "digit %u of %zu bins", d, h.size());
            h[d] += 1;
            if (pass == 0 && w1 == TOPK_W1) { CHECK(topk_first_slot(d) < (uint32_t)TOPK_BINS1, "slot"); slots[topk_first_slot(d)] += 1; }
        }
        if (pass == 0 && w1 == TOPK_W1)       // wave 0 reads vector q * 64 + l of lane l as bins 16 l + 4 q + e
            for (uint32_t d = 0; d < h.size(); ++d)
                CHECK(slots[4 * (((d >> 2) & 3) * 64 + (d >> 4)) + (d & 3)] == h[d], "first-pass slot of bin %u", d);
        uint32_t cum = 0, b = 0;
        while (cum + h[b] < remaining) { cum += h[b]; ++b; CHECK(b < h.size(), "ran off the histogram"); if (b >= h.size()) return s; }
        T |= b << shift;
        remaining -= cum;
        eq_total = h[b];
        top = shift;
        if (pass == 0) s.excess = (long)eq_total - (long)remaining;
        ++pass;
        if (eq_total == remaining) break;
    }
    if (pass == 0) eq_total = remaining + 1u;
    s.T = T; s.lim = topk_winner_limit(rg.span, T, top); s.remaining = remaining; s.eq_total = eq_total; s.passes = pass;
    CHECK(eq_total == remaining || top == 0, "an undecided bit with an unresolved bucket");
    return s;
}

// ---- the rule this one replaced (here only): real keys, 8-bit digits below the highest bit in which kmin and bound differ
static Sel select_xor_prefix(const std::vector<float>& v, int k, int nthr) {
    const int N = (int)v.size();
    uint32_t kmin, bound;
    key_range(v, k, nthr, kmin, bound);
    const uint32_t diff = kmin ^ bound;
    int top = topk_bit_length(diff);
    uint32_t T = top >= 32 ? 0u : (kmin >> top) << top, remaining = (uint32_t)k, eq_total = (uint32_t)N;
    Sel s;
    int pass = 0;
    while (top > 0) {
        const int width = top >= 8 ? 8 : top, shift = top - width;
        uint32_t h[256] = {0};
        for (int n = 0; n < N; ++n) {
            const uint32_t key = reward_key(v[n]);
            if (top >= 32 || (key >> top) == (T >> top)) h[(key >> shift) & ((1u << width) - 1u)] += 1;
        }
        uint32_t cum = 0, b = 0;
        while (cum + h[b] < remaining) { cum += h[b]; ++b; }
        T |= b << shift;
        remaining -= cum;
        eq_total = h[b];
        top = shift;
        if (pass == 0) s.excess = (long)eq_total - (long)remaining;
        ++pass;
        if (eq_total == remaining) break;
    }
    s.passes = pass;
    return s;
}

// ---- winners of a selection: topk_is_winner for every element (ascending index), then block_topk_finish_sorted's order
static void winners(const std::vector<float>& v, const Sel& s, std::vector<int>& by_index, std::vector<int>& sorted) {
    const int N = (int)v.size();
    by_index.clear();
    uint32_t ties_ahead = 0;
    for (int n = 0; n < N; ++n) {
        const uint32_t kp = topk_offset_key(v[n], s.kmin);
        bool in;
        if (s.eq_total == s.remaining) in = kp <= s.lim;
        else if (kp < s.T) in = true;
        else if (kp != s.T) in = false;
        else { in = ties_ahead < s.remaining; ++ties_ahead; }
        if (in) by_index.push_back(n);
    }
    std::vector<unsigned long long> w;
    for (int n : by_index) w.push_back(((unsigned long long)topk_offset_key(v[n], s.kmin) << 32) | (uint32_t)n);
    std::sort(w.begin(), w.end());
    sorted.clear();
    for (unsigned long long x : w) sorted.push_back((int)(uint32_t)(x & 0xFFFFFFFFull));
}

static bool better(float a, float b) { return a > b; }          // (-0 == +0: a tie, as the keys have it)

static void check_population(const std::vector<float>& v, int k, int nthr, const char* what, int w1 = TOPK_W1) {
    const int N = (int)v.size();
    const Sel s = select_offset(v, k, nthr, w1);
    CHECK(s.passes <= 1 + (32 - w1 + 7) / 8, "%s N %d k %d: %d passes", what, N, k, s.passes);
    std::vector<int> by_index, sorted;
    winners(v, s, by_index, sorted);
    std::vector<int> ref(N);
    for (int n = 0; n < N; ++n) ref[n] = n;
    std::stable_sort(ref.begin(), ref.end(), [&](int a, int b) { return better(v[a], v[b]); });
    ref.resize(k);
    CHECK(sorted == ref, "%s N %d k %d nthr %d: sorted order differs (%zu winners)", what, N, k, nthr, sorted.size());
    std::sort(ref.begin(), ref.end());
    CHECK(by_index == ref, "%s N %d k %d nthr %d: winner set differs", what, N, k, nthr);
}

// a small generator of its own: the populations must not depend on the C++ library
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint32_t u32() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    double uni() { return (u32() + 0.5) / 4294967296.0; }
    float normal() { return (float)(std::sqrt(-2.0 * std::log(uni())) * std::cos(6.283185307179586 * uni())); }
};

static const char* kinds[] = {"normal", "all equal", "two values", "+-0 mixed", "-1e6 mixed", "+-inf", "denormals", "tie group"};

static std::vector<float> population(int kind, int N, int k, Rng& r) {
    std::vector<float> v(N);
    const float inf = std::numeric_limits<float>::infinity();
    for (int n = 0; n < N; ++n) {
        const float g = -100.0f + 30.0f * r.normal();
        switch (kind) {
            case 0: v[n] = g; break;
            case 1: v[n] = -3.25f; break;
            case 2: v[n] = (r.u32() & 1) ? -1.0f : -2.0f; break;
            case 3: v[n] = (r.u32() % 3 == 0) ? 0.0f : ((r.u32() & 1) ? -0.0f : (r.u32() % 5 == 0 ? -1.0f : 0.0f)); break;
            case 4: v[n] = (r.u32() % 3 == 0) ? -1.0e6f : g; break;                      // span near 2^31
            case 5: v[n] = (r.u32() % 4 == 0) ? inf : ((r.u32() % 4 == 0) ? -inf : g); break;
            case 6: v[n] = (float)((int)(r.u32() % 41) - 20) * 1.0e-41f; break;          // denormals of both signs, and zeros
            default: v[n] = g; break;
        }
    }
    if (kind == 7 && N >= 2) {       // a group of equal rewards across the k-th place: the (k-1)-th best lends its value
        std::vector<float> s(v);
        std::sort(s.begin(), s.end(), better);
        const float val = s[std::max(0, std::min(N - 1, k - 1) - (int)(r.u32() % 3))];
        const int g = 1 + (int)(r.u32() % (uint32_t)std::min(N, 70));
        for (int i = 0; i < g; ++i) v[r.u32() % (uint32_t)N] = val;
    }
    return v;
}

static int threads_for(int N, int k) { return std::min(1024, std::max(64, ((std::max(N, k) + 63) / 64) * 64)); }

static int run_checks() {
    Rng r(12345);
    for (int N = 1; N <= 1100; ++N) {
        const int ks[5] = {1, 2, 50, 64, N};
        for (int ki = 0; ki < 5; ++ki) {
            const int k = ks[ki];
            if (k > N || (ki == 4 && (N == 1 || N == 2 || N == 50 || N == 64))) continue;     // (k = N: once)
            for (int kind = 0; kind < 8; ++kind) {
                const std::vector<float> v = population(kind, N, k, r);
                check_population(v, k, threads_for(N, k), kinds[kind]);
                if (N % 97 == 0) check_population(v, k, 64, kinds[kind]);               // one wave: many elements per lane
                if (N % 7 == 0) check_population(v, k, 1024, kinds[kind], TOPK_WN);     // the narrow form (CMA-ES kernels)
            }
        }
    }
    // ---- pass counts
    {
        const int N = 500, k = 50, nthr = 512;
        std::vector<float> v(N);
        for (int n = 0; n < N; ++n) v[n] = -127.5f - (float)n / (float)(N - 1);          // evenly spaced over -128 +- 0.5
        const Sel a = select_offset(v, k, nthr), b = select_xor_prefix(v, k, nthr);
        CHECK(a.passes == 1, "evenly spaced over -128 +- 0.5: %d passes (excess %ld)", a.passes, a.excess);
        CHECK(b.passes >= 2, "the old rule on the same population: %d passes", b.passes);
        check_population(v, k, nthr, "evenly spaced");
        std::vector<float> w(v);                                                        // the same rewards in another order
        Rng q(7);
        for (int n = N - 1; n > 0; --n) std::swap(w[n], w[q.u32() % (uint32_t)(n + 1)]);
        const Sel c = select_offset(w, k, nthr);
        CHECK(c.passes == 1, "evenly spaced, shuffled: %d passes", c.passes);
        check_population(w, k, nthr, "evenly spaced, shuffled");
        printf("evenly spaced over -128 +- 0.5: %d pass (old rule %d, %ld keys too many in its first bucket)\n", a.passes, b.passes, b.excess);
    }
    {
        std::vector<float> v(300, -7.0f);
        CHECK(select_offset(v, 50, 320).passes == 0, "span == 0 must take no pass");
        v[299] = -9.0f;                  // 19 rows of two give the bound for k = 30: a row's second minimum, the tied value
        CHECK(select_offset(v, 30, 320).passes == 0, "span == 0 (one worse key) must take no pass");
        check_population(v, 30, 320, "span == 0");
    }
    CHECK(TOPK_MAX_PASSES == 1 + (32 - TOPK_W1 + 7) / 8, "pass bound");
    CHECK(TOPK_HIST_WORDS == TOPK_BINS1 + 16 + 256 && TOPK_HIST_WORDS % 4 == 0 && TOPK_HIST_WORDS_NARROW == 528, "LDS words");
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("all checks held\n");
    return 0;
}

static int run_passes(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) { printf("cannot open %s\n", path); return 2; }
    int32_t hdr[4];
    if (fread(hdr, 4, 4, f) != 4) { fclose(f); return 2; }
    const int M = hdr[0], N = hdr[1], k = hdr[2], nthr = hdr[3];
    if (M < 0 || N < 1 || k < 1 || k > N || nthr < 64 || nthr % 64) { fclose(f); printf("bad header\n"); return 2; }
    std::vector<float> v(N);
    for (int m = 0; m < M; ++m) {
        if (fread(v.data(), 4, (size_t)N, f) != (size_t)N) { fclose(f); printf("short file\n"); return 2; }
        const Sel a = select_offset(v, k, nthr), b = select_xor_prefix(v, k, nthr);
        printf("%d %ld %d %ld\n", a.passes, a.excess, b.passes, b.excess);
    }
    fclose(f);
    return g_fail ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "--passes")) return run_passes(argv[2]);
    return run_checks();
}
