// Stand-alone check of blackbox_mpc_amd/csrc/noise_extent.hpp (plain C++, own main; run by tests/test_noise_extent_cpu.py).
//
// The persistent pendulum kernel's prefetched-draws rollout walks a pointer along a trajectory's row of float4 blocks and
// loads ahead of its use with no clamp at the row's end.  Here the loop's control flow is restated with the loads alone
// (walk()), every index it touches is recorded, and for a grid of shapes:
//   * the header's extent equals the highest index the walk touches, for every trajectory, agent and iteration;
//   * every block a model step USES lies inside the trajectory's own row;
//   * no index, in any control step of a chunk buffer, reaches the end of the padded allocation, and the last row of
//     the last step reaches exactly into the pad when the header says there is one;
//   * the pad is at most two float4.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../blackbox_mpc_amd/csrc/noise_extent.hpp"

using namespace bbmpc;

static int g_fail = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++g_fail < 20) { printf("FAILED %s: ", #c); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Walk { size_t hi_read = 0, hi_used = 0; };

// the CEM / PI2 / RandomSearch loop of kernels_fused.hpp (INJ == 2), loads and uses only; row = index of the row's block 0
static Walk walk(size_t row, int H) {
    Walk w;
    const int nblk = H >> 2, rem = H & 3;
    auto read = [&](size_t i) { if (i > w.hi_read) w.hi_read = i; };
    auto use = [&](size_t i) { if (i > w.hi_used) w.hi_used = i; };
    w.hi_read = w.hi_used = row;
    read(row + 0); read(row + 1);                 // c0, c1 (or prefetch_first's q[0], q[1]: the same two)
    size_t c0 = row, c1 = row + 1;                // which block each register pair holds
    size_t at = row;                              // the block the code is at
    for (int trips = nblk >> 1; trips > 0; --trips) {
        use(c0); read(at + 2); c0 = at + 2;       // block4(c0, 0, ., true)
        use(c1); read(at + 3); c1 = at + 3;       // block4(c1, 1, ., true)
        at += 2;
    }
    if (nblk & 1) { use(c0); c0 = c1; at += 1; }  // block4(c0, 2, ., false)
    if (rem > 0) use(c0);
    (void)at;
    return w;
}

// the SPSA loop
static Walk walk_spsa(size_t row, int H) {
    Walk w;
    const int nb4 = (H + 3) >> 2;
    w.hi_read = w.hi_used = row;
    size_t cur = row;
    for (int b = 0; b < nb4; ++b) {
        const size_t nxt = row + (size_t)b + 1;
        if (nxt > w.hi_read) w.hi_read = nxt;
        if (cur > w.hi_used) w.hi_used = cur;
        cur = nxt;
    }
    return w;
}

int main() {
    const int Hs[] = {1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 30, 31};
    const int Ns[] = {1, 63, 64, 70, 500, 512};
    const int As[] = {1, 2, 3};
    const int Its[] = {1, 3, 5};
    const int steps = 8;                          // control steps per chunk buffer
    long cases = 0;
    for (int H : Hs) for (int N : Ns) for (int A : As) for (int iters : Its) {
        const int Nst = ((N + 63) / 64) * 64, Q = (H + 3) >> 2;
        const size_t step_f4 = noise_step_floats(iters, A, Nst, H) / 4;
        const size_t alloc_f4 = noise_alloc_floats(steps, iters, A, Nst, H) / 4;
        CHECK(noise_step_floats(iters, A, Nst, H) == (size_t)iters * A * Nst * Q * 4, "H=%d", H);
        CHECK(noise_alloc_floats(steps, iters, A, Nst, H) % 4 == 0, "H=%d", H);
        CHECK(alloc_f4 == step_f4 * steps + (size_t)noise_pad_blocks(H), "H=%d", H);
        CHECK(noise_pad_blocks(H) >= 0 && noise_pad_blocks(H) <= 2, "H=%d pad=%d", H, noise_pad_blocks(H));
        size_t top = 0;
        for (int spsa = 0; spsa < 2; ++spsa)
            for (int it = 0; it < iters; ++it) for (int a = 0; a < A; ++a) for (int n = 0; n < N; ++n) {
                const size_t row = noise_block_index(it, A, a, Nst, n, Q);
                const Walk w = spsa ? walk_spsa(row, H) : walk(row, H);
                const size_t ext = noise_extent_index(it, A, a, Nst, n, Q, H, spsa != 0);
                CHECK(w.hi_read == ext, "H=%d N=%d A=%d it=%d a=%d n=%d spsa=%d: walk %zu header %zu", H, N, A, it, a, n, spsa, w.hi_read, ext);
                CHECK(w.hi_used <= row + (size_t)Q - 1, "H=%d n=%d spsa=%d: a model step uses block %zu past its row", H, n, spsa, w.hi_used - row);
                CHECK(ext <= row + (size_t)Q - 1 + 2, "H=%d: more than two float4 past the row", H);
                // every control step of the chunk, the last one included: inside the padded allocation
                CHECK((size_t)(steps - 1) * step_f4 + ext < alloc_f4, "H=%d N=%d A=%d iters=%d it=%d a=%d n=%d spsa=%d: %zu >= %zu", H, N, A, iters, it, a, n, spsa,
                      (size_t)(steps - 1) * step_f4 + ext, alloc_f4);
                if (ext > top) top = ext;
                ++cases;
            }
        // the last trajectory of the last agent in the last iteration of the last step: with no slack rows (N == Nst)
        // the highest index read is exactly the allocation's last float4 -- the pad is as small as it can be
        if (N == Nst) CHECK((size_t)(steps - 1) * step_f4 + top == alloc_f4 - 1, "H=%d N=%d: top %zu alloc %zu", H, N, (size_t)(steps - 1) * step_f4 + top, alloc_f4);
    }
    if (g_fail) { printf("%d checks FAILED\n", g_fail); return 1; }
    printf("%ld trajectories walked\nall checks held\n", cases);
    return 0;
}
