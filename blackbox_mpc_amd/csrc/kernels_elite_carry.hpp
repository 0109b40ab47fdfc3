// Elite carry-over for CEM (bbmpc_set_elite_carry): the best few elites of an iteration are put back
// among the candidates of the next one (keep), and the best few of a control step's last iteration, moved one planning
// step forward, among the candidates of the next control step's first iteration (shift).
//
//   k_elite_save    after a refit: rows E[a][0 .. count) of the sample buffer -> the handle's carry buffer [A][HU][Kc]
//   k_elite_inject  after the next draw: the first `count` columns of the carry buffer -> the LAST `count` candidates
//
// Two launches, not one: the draw that lies between them rewrites every column of the sample buffer, so the elite rows
// have to leave it before the draw and can only come back after it.  Both are launch-latency kernels (at most
// HU * num_elite elements per agent): thread = (row j, elite e), e fastest, so the carry buffer is read and written in
// address order; every global pointer is a `__restrict__` kernel argument of its own (the reason kernels_corr.hpp gives),
// the elite index is read once per thread, no LDS, no scratch.
#pragma once
#include <hip/hip_runtime.h>

namespace bbmpc {

constexpr int CARRY_THREADS = 256;

// grid (ceil(HU * count / 256), A).  elites [A][k] sorted best first (k_refit_cem / k_refit_cem_v2), samples [A][HU][Nst].
// SHIFT: row j = t * U + u goes to row j - U (planning step t -> t - 1) and the last planning step is also written in
// place, i.e. repeated; the first planning step is dropped.
template <bool SHIFT>
__global__ __launch_bounds__(CARRY_THREADS) void k_elite_save(int HU, int U, int Nst, int N, int k, int Kc, int count,
                                                              const int* __restrict__ elites, const float* __restrict__ samples,
                                                              float* __restrict__ carry) {
    const int a = blockIdx.y, idx = blockIdx.x * CARRY_THREADS + threadIdx.x;
    if (idx >= HU * count) return;
    const int j = idx / count, e = idx - j * count;
    // (the selection only lists candidates of the population; the clamp keeps a damaged list inside the buffer)
    const int n = min(max(elites[a * k + e], 0), N - 1);
    const float v = samples[((size_t)a * HU + j) * Nst + n];
    if constexpr (SHIFT) {
        if (j >= U) carry[((size_t)a * HU + j - U) * Kc + e] = v;
        if (j >= HU - U) carry[((size_t)a * HU + j) * Kc + e] = v;
    } else {
        carry[((size_t)a * HU + j) * Kc + e] = v;
    }
}

// grid (ceil(HU * count / 256), A), count < N: carry column e -> candidate N - count + e, bit for bit.
static __global__ __launch_bounds__(CARRY_THREADS) void k_elite_inject(int HU, int Nst, int N, int Kc, int count, const float* __restrict__ carry,
                                                                float* __restrict__ samples) {
    const int a = blockIdx.y, idx = blockIdx.x * CARRY_THREADS + threadIdx.x;
    if (idx >= HU * count) return;
    const int j = idx / count, e = idx - j * count;
    samples[((size_t)a * HU + j) * Nst + (N - count + e)] = carry[((size_t)a * HU + j) * Kc + e];
}

}  // namespace bbmpc
