// Temporally correlated candidates for CEM / PI2 (bbmpc_set_sampling_correlation): the standard
// truncated-normal draws z[s] of a candidate are mixed along the time axis by one H x H matrix before the affine step
//   y[t,u] = sum_s M[t,s] * z[s,u]   (s ascending, fp32, one rounding per product and per sum)
//   x[t,u] = y * sigma[t,u] + mean[t,u]                       -- candidate<SRC_TRUNC>'s expression: M = I gives its bits
// and, for CEM, clipped to the action bounds (a mixed draw is no longer bounded by two sigma).  The result goes to the
// sample buffer, from where the SRC_BUF form of every rollout kernel reads it (Engine::launch_rollout).
//
// One wave per workgroup, lane = candidate.  A lane keeps its H*U draws in an LDS tile [HU][64]: lane-minor, so the wave
// reads one 256-byte row per ds_read_b32 (lanes l and l+32 share a bank but sit in different halves: conflict-free) and a
// lane only ever reads what it wrote itself -- no barrier.  M, sigma and the mean are wave-uniform and come through
// `const float* __restrict__`, i.e. scalar loads; per row t the host passes the index after the last non-zero column, so a
// lower-triangular M costs half (the skipped terms are exact zeros behind the last non-zero one: the sum keeps its bits).
#pragma once
#include <hip/hip_runtime.h>

#include "kernels_rollout.hpp"
#include "models.hpp"

namespace bbmpc {

constexpr int CORR_LANES = 64;
constexpr int CORR_CHUNK = 8;                                     // terms whose operands are fetched together
constexpr int CORR_MAX_HU = 159 * 1024 / (CORR_LANES * 4);        // the tile has to fit one CU's LDS: H*U <= 636

// grid (ceil(n_pop/64), A), block 64, LDS HU * 64 floats.  Everything the mixing loop reads or writes in global memory is a
// `__restrict__` kernel argument of its own (not a member of `p`): only then may the compiler keep the wave-uniform reads of
// M, sigma, the mean and the bounds on the scalar unit while the loop stores samples (read through `p` they are vector
// loads queued behind the stores).
template <bool CLIP>
__global__ __launch_bounds__(CORR_LANES) void k_gen_candidates_corr(RolloutArgs p, const float* __restrict__ mix,
                                                                    const int* __restrict__ row_end, const float* __restrict__ mean_all,
                                                                    const float* __restrict__ sigma_all, const float* __restrict__ lo,
                                                                    const float* __restrict__ hi, float* __restrict__ samples) {
    extern __shared__ float ztile[];                               // [HU][64]
    const int a = blockIdx.y, lane = threadIdx.x, n = blockIdx.x * CORR_LANES + lane;
    const bool active = n < p.n_pop;
    const float* __restrict__ mean = mean_all + (size_t)a * p.HU;
    const float* __restrict__ sigma = sigma_all + (size_t)a * p.HU;
    // the unmixed draws, keyed exactly as candidate<SRC_TRUNC> keys them (or the injected tensor)
    U4 blk = {0, 0, 0, 0};
    for (int j = 0; j < p.HU; ++j) {
        float xi = 0.0f;
        if (active) {
            if (p.inj) {
                xi = p.inj[((size_t)a * p.HU + j) * p.Nst + n];
            } else {
                if ((j & 3) == 0) blk = rng_block(p.key, p.stream, p.iter, (uint32_t)(n + p.pop_offset), (uint32_t)(p.agent_offset + a), (uint32_t)j);
                xi = word_to_trunc_normal(pick_word(blk, (uint32_t)j));
            }
        }
        ztile[j * CORR_LANES + lane] = xi;
    }
    for (int t = 0; t < p.H; ++t) {
        const float* __restrict__ row = mix + (size_t)t * p.H;
        const int e = row_end[t];                                  // >= 1
        for (int u = 0; u < p.U; ++u) {
            const int j = t * p.U + u;
            float y = row[0] * ztile[u * CORR_LANES + lane];
            // eight terms' operands at a time: the scalar loads of M and the LDS reads of z count on one counter, so a
            // term-by-term loop would wait for both once per term; the sum itself stays one dependent chain in s order
            for (int s0 = 1; s0 < e; s0 += CORR_CHUNK) {
                float m[CORR_CHUNK], z[CORR_CHUNK];
#pragma unroll
                for (int i = 0; i < CORR_CHUNK; ++i) {
                    const int s = min(s0 + i, p.H - 1);            // (past the row's end: a valid address, the term is not added)
                    m[i] = row[s];
                    z[i] = ztile[(s * p.U + u) * CORR_LANES + lane];
                }
#pragma unroll
                for (int i = 0; i < CORR_CHUNK; ++i)
                    if (s0 + i < e) y = y + m[i] * z[i];
            }
            float x = y * sigma[j] + mean[j];
            if constexpr (CLIP) x = clipf(x, lo[u], hi[u]);
            if (active) samples[((size_t)a * p.HU + j) * p.Nst + n] = x;
        }
    }
}

}  // namespace bbmpc
