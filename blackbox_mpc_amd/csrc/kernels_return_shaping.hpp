// Discounted, termination-aware returns of the learned-model rollouts (bbmpc_set_return_shaping).
//
// The rollouts in front of this kernel have recorded the state after every step in u_traj [H][A][Nst][S] and left
// -(bound penalty) in `rewards`.  Per candidate n of agent a, with s_0 the agent's state, s_{t+1} = plane t, a_t the
// candidate buffer behind the rollout (the clipped actions), r_t either reward_generic (a built-in reward) or step[t]
// (what k_reward_mlp_traj wrote for a learned reward):
//     g = 1; alive = true; R = 0; T = 0
//     for t = 0 .. H-1:   R += g * r_t
//                         if outside(s_{t+1}):  R += g * c; alive = false; T = t + 1; stop
//                         g *= gamma
//     if isnan(R): R = -1e6
//     R += rewards[a][n]
//     if alive and vterm:  R = R + (g * w) * vterm[a][n];  a NaN term -> R = -1e6
// outside(s) = any i: s[i] < lo[i] or s[i] > hi[i]; both comparisons are false on NaN, so a NaN state does not terminate.
// What lies behind the terminal step is never read into R: the lane is switched off (a select, no multiplication by zero).
//
// Work split: one wave per workgroup owns 64 consecutive candidates of one agent (grid = ceil(n_pop / 64) x A).  The
// walk over t is serial per candidate and candidates are independent, so there is nothing to reduce and no atomic.  The
// 64 rows of a plane are 64 * S contiguous floats: the wave streams them into an LDS tile with consecutive lanes on
// consecutive addresses (global_load_dwordx4 where S % 4 == 0) and every lane then reads its own row from LDS, rows
// S | 1 floats apart (an odd stride: 64 lanes on 64 different banks).  Two tiles, s_t and s_{t+1}, change places every
// step; a built-in reward that reads actions gets a third tile [64][U | 1].  Rows n >= n_pop are neither read nor
// written.  The wave stops reading planes once all of its candidates have terminated.
#pragma once
#include "models.hpp"

namespace bbmpc {

constexpr int SHAPED_LANES = 64;

struct ShapedReturnArgs {
    int n_pop, A, H, Nst, HU, S, U;
    int from_ref;                    // SRC_REF: actions from seq, else from cand
    int reward_kind, fix_q1;         // read when step == nullptr: reward_generic's arguments
    float gamma, term_reward, weight;
    const float* state;              // [A][S]
    const float* traj;               // [H][A][Nst][S] the state after every step
    const float* seq;                // SRC_REF: [n_pop][A][HU]
    const float* cand;               // else: [A][HU][Nst]
    const float* step;               // [H][A][Nst] per-step rewards (BBMPC_REW_MLP), or nullptr
    const float* vterm;              // [A][Nst] V of the last plane, or nullptr
    const float* box;                // [2][S]: lo | hi, -inf / +inf = unbounded
    float* rewards;                  // [A][Nst]: -(penalty) in, the shaped score out
    int* tsteps;                     // [A][Nst]: the first terminal step in 1 .. H, 0 = none
};

// floats of dynamic LDS: two state tiles and the action tile
__host__ __device__ inline int shaped_return_lds_floats(int S, int U) { return SHAPED_LANES * (2 * (S | 1) + (U | 1)); }

#ifdef BBMPC_TU_MLP

// `rows` rows of S floats at src (contiguous) -> tile rows ld apart; V4: S % 4 == 0 and src 16-byte aligned
template <bool V4>
__device__ __forceinline__ void shaped_load_rows(const float* __restrict__ src, float* tile, int rows, int S, int ld, int lane) {
    if (V4) {
        const float4* src4 = reinterpret_cast<const float4*>(src);
        const int n4 = rows * (S >> 2);
        for (int i = lane; i < n4; i += SHAPED_LANES) {
            const float4 v = src4[i];
            const int e = i << 2, r = e / S, c = e - r * S;       // (the four elements lie in one row: S % 4 == 0)
            float* d = tile + r * ld + c;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        }
    } else {
        const int n = rows * S;
        for (int i = lane; i < n; i += SHAPED_LANES) {
            const int r = i / S, c = i - r * S;
            tile[r * ld + c] = src[i];
        }
    }
}

template <bool V4>
__global__ __launch_bounds__(SHAPED_LANES) void k_shaped_return(ShapedReturnArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = threadIdx.x, a = blockIdx.y, n0 = blockIdx.x * SHAPED_LANES, n = n0 + lane;
    const int S = q.S, U = q.U, ld = S | 1, lu = U | 1;
    const int rows = min(SHAPED_LANES, q.n_pop - n0);             // >= 1 by the grid
    float* cur = smem;
    float* nxt = smem + SHAPED_LANES * ld;
    float* acts = smem + 2 * SHAPED_LANES * ld;
    const float* __restrict__ lo = q.box;
    const float* __restrict__ hi = q.box + S;
    const bool need_act = q.step == nullptr && q.reward_kind != REW_NONE;
    for (int i = lane; i < rows * S; i += SHAPED_LANES) {         // s_0: the agent's state in every row
        const int r = i / S, c = i - r * S;
        cur[r * ld + c] = q.state[(size_t)a * S + c];
    }
    bool active = n < q.n_pop;
    float g = 1.0f, R = 0.0f;
    int T = 0;
    // what moves with t is walked, not recomputed: the tile's rows of plane t, the lane's step reward and its actions
    const float* plane = q.traj + ((size_t)a * q.Nst + n0) * S;
    const size_t plane_stride = (size_t)q.A * q.Nst * S, step_stride = (size_t)q.A * q.Nst;
    const float* stepp = q.step ? q.step + (size_t)a * q.Nst + n : nullptr;
    const float* actp = q.from_ref ? q.seq + ((size_t)n * q.A + a) * q.HU : q.cand + (size_t)a * q.HU * q.Nst + n;
    const int act_stride = q.from_ref ? 1 : q.Nst;                // between consecutive (t, u) of one candidate
    for (int t = 0; t < q.H; ++t) {
        if (__ballot(active) == 0) break;                         // (one wave: uniform)
        shaped_load_rows<V4>(plane, nxt, rows, S, ld, lane);
        if (need_act && active)
            for (int u = 0; u < U; ++u) acts[lane * lu + u] = actp[(size_t)u * act_stride];
        __syncthreads();
        if (active) {
            const float* c = cur + lane * ld;
            const float* x = nxt + lane * ld;
            const float r = stepp ? *stepp : reward_generic(q.reward_kind, q.fix_q1 != 0, c, acts + lane * lu, x, S, U);
            R = R + g * r;
            bool out = false;
            for (int i = 0; i < S; ++i) {
                const float v = x[i];
                out = out || v < lo[i] || v > hi[i];
            }
            if (out) {
                R = R + g * q.term_reward;
                T = t + 1;
                active = false;
            } else {
                g = g * q.gamma;
            }
        }
        __syncthreads();
        float* sw = cur; cur = nxt; nxt = sw;
        plane += plane_stride;
        if (stepp) stepp += step_stride;
        actp += (size_t)U * act_stride;
    }
    if (n >= q.n_pop) return;
    const size_t o = (size_t)a * q.Nst + n;
    if (R != R) R = -1.0e6f;
    R = R + q.rewards[o];
    if (T == 0 && q.vterm) {                                      // alive: the horizon closes with g = gamma^H
        const float term = (g * q.weight) * q.vterm[o];
        R = R + term;
        if (term != term) R = -1.0e6f;
    }
    q.rewards[o] = R;
    q.tsteps[o] = T;
}

#endif  // BBMPC_TU_MLP

}  // namespace bbmpc
