// Open-loop trajectory prediction through the learned model (bbmpc_predict_trajectories): the generic MFMA rollout's
// recurrence (kernels_mlp.hpp, SPEC 0: v_mfma_f32_16x16x4_f32, fp32 in / fp32 accumulate, operands streamed from the
// packed [OT][IT][lane][4] copy, run-time activation codes) with a different frame around it:
//   - a workgroup owns 16 ROWS of the batch, each with its own start state (no agents, no candidates, no penalty);
//   - the action row of step t + 1 is fetched from global memory while step t's Dense stack runs -- two registers per
//     thread, written to LDS behind the stack -- so Hq is not bounded by an LDS action block;
//   - after every step the 16 x S state tile goes from LDS to states_out[B, Hq, S] (a row's S floats are contiguous:
//     16 segments of 4 S bytes per step) and the step's reward to rewards_out[B, Hq]; nothing is summed, no NaN rule.
// The prologue (normalisation constants, state / input staging) and the epilogue (partial sums, bias, de-normalise,
// residual) restate rollout_mlp_body<0> of kernels_mlp.hpp, which must keep compiling to what it compiles to: a fix in one
// of the two belongs in the other as well.  Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp.hpp"

namespace bbmpc {

struct MlpTrajArgs {
    MlpDesc m;
    const float* wp4[MLP_MAX_LAYERS];    // MlpRolloutArgs::wp4
    int nw;                              // waves per workgroup
    int B, Hq, S, U;
    int reward_kind, fix_q1;
    const float* states;                 // [B, S]
    const float* seq;                    // [B, Hq, U]
    float* states_out;                   // [B, Hq, S] or null
    float* rewards_out;                  // [B, Hq] or null
};

// LDS carve in floats (pieces are multiples of 4 floats): the rollout's xs / actA / actB / part / st, then
//   acts [2][16][U]   the actions of step t and t + 1
//   norm              as MlpLds::norm
struct MlpTrajLds {
    int xs, actA, actB, part, st, acts, norm, total;
};
__host__ __device__ inline MlpTrajLds mlp_traj_lds_layout(const MlpDesc& m, int U, int S, int nw) {
    MlpTrajLds l;
    int itmax = 1;
    for (int i = 1; i < m.n_layers; ++i) itmax = itmax > m.tiles[i] ? itmax : m.tiles[i];
    const int Sp = (S + 3) & ~3;
    int o = 0;
    l.xs = o;   o += m.tiles[0] * 256;
    l.actA = o; o += itmax * 256;
    l.actB = o; o += itmax * 256;
    l.part = o; o += nw * m.tiles[m.n_layers] * 256;
    l.st = o;   o += 2 * MLP_TP * Sp;
    l.acts = o; o += ((2 * MLP_TP * U + 3) & ~3);
    l.norm = o; o += (((S + U) * 2 + S * 3 + 63) & ~63);
    l.total = o;
    return l;
}

constexpr int MLP_TRAJ_PF = 2;      // action elements a thread holds in registers across a step's Dense stack

template <bool EXT>
__global__ void k_traj_mlp(MlpTrajArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& m = q.m;
    const int n0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = q.S, U = q.U, Hq = q.Hq, L = m.n_layers, B = q.B;
    const int Sp = (S + 3) & ~3;
    const MlpTrajLds lay = mlp_traj_lds_layout(m, U, S, nw);
    float* xs = smem + lay.xs;
    float* part = smem + lay.part;
    float* st = smem + lay.st;
    float* acts = smem + lay.acts;
    const bool normd = m.normalized != 0;
    float* nmean = smem + lay.norm;             // [S+U] input means (0 when not normalised)
    float* ninv = nmean + (S + U);              // [S+U] 1/(std + 1e-7)   (1 when not normalised)
    float* tmean = ninv + (S + U);              // [S] target mean
    float* tstd = tmean + S;                    // [S] target std + 1e-7
    float* lbias = tstd + S;                    // [S] bias of the last layer

    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? m.mean_s[f] : m.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? m.std_s[f] : m.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;          // system_dynamics_handler.py:119-122 (x - mu)/(sd + 1e-7)
        if (f < S) {
            tmean[f] = normd ? m.mean_t[f] : 0.0f;
            tstd[f] = normd ? (m.std_t[f] + 1e-7f) : 1.0f;
            lbias[f] = m.bpack[L - 1][((size_t)(f >> 4) * 64 + ((f & 15) >> 2) * 16) * 4 + (f & 3)];
        }
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) xs[i] = 0.0f;
    for (int i = tid; i < MLP_TP * S; i += nthr) {
        const int pp = i / S, s = i % S;
        st[pp * Sp + s] = (n0 + pp < B) ? q.states[(size_t)(n0 + pp) * S + s] : 0.0f;
    }
    for (int e = tid; e < MLP_TP * U; e += nthr) {                 // the actions of step 0 (rows past the batch roll zeros)
        const int pp = e / U, u = e % U;
        acts[e] = (n0 + pp < B) ? q.seq[((size_t)(n0 + pp) * Hq) * U + u] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < MLP_TP * (S + U); i += nthr) {          // normalised layer-0 input for t = 0
        const int f = i / MLP_TP, pp = i % MLP_TP;
        const float v = (f < S) ? st[pp * Sp + f] : acts[pp * U + (f - S)];
        xs[tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
    }
    __syncthreads();

    const int OTl = m.tiles[L];
    for (int t = 0; t < Hq; ++t) {
        float* cur = st + (t & 1) * MLP_TP * Sp;
        float* nxt = st + ((t + 1) & 1) * MLP_TP * Sp;
        const float* act_t = acts + (t & 1) * MLP_TP * U;
        float* act_n = acts + ((t + 1) & 1) * MLP_TP * U;
        const bool more = t + 1 < Hq;
        // ---- the next step's action elements e = tid, tid + nthr of the tile [16][U]: in flight across the Dense stack
        float pf[MLP_TRAJ_PF];
#pragma unroll
        for (int j = 0; j < MLP_TRAJ_PF; ++j) {
            const int e = tid + j * nthr;
            const int pp = e / U, u = e - pp * U;
            pf[j] = (more && e < MLP_TP * U && n0 + pp < B) ? q.seq[((size_t)(n0 + pp) * Hq + (t + 1)) * U + u] : 0.0f;
        }
        // ---- dense layers (kernels_mlp.hpp, SPEC 0)
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            mlp_layer_out_split<EXT>(m, q.wp4[l], l, in_off, out_off, wave, lane, nw);
            __syncthreads();
            in_off = out_off;
        }
        mlp_layer_k_split(m, q.wp4[L - 1], L - 1, in_off, lay.part, wave, lane, nw);
        __syncthreads();
        // ---- epilogue: reduce partials, bias, last activation, de-normalise, residual; stage step t + 1's input
        const int nwp = min(nw, m.tiles[L - 1]);          // waves that actually produced partials
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int f = i / MLP_TP, pp = i % MLP_TP;
            const int ot = f >> 4, ln = ((f & 15) >> 2) * 16 + pp, rg = f & 3;
            const float* pp0 = part + (((size_t)ot) * 64 + ln) * 4 + rg;
            float acc = lbias[f];
            for (int w = 0; w < nwp; ++w) acc = acc + pp0[(size_t)w * OTl * 256];
            acc = apply_act_rt<EXT>(acc, m.act[L - 1]);
            const float dev = normd ? tmean[f] + acc * tstd[f] : acc;       // system_dynamics_handler.py:152-155
            const float ns = dev + cur[pp * Sp + f];                        // transforms.py:34
            nxt[pp * Sp + f] = ns;
            xs[tile_addr(f, pp)] = (ns - nmean[f]) * ninv[f];
        }
        if (more) {
#pragma unroll
            for (int j = 0; j < MLP_TRAJ_PF; ++j) {
                const int e = tid + j * nthr;
                if (e < MLP_TP * U) {
                    const int pp = e / U, u = e - pp * U;
                    act_n[e] = pf[j];
                    xs[tile_addr(S + u, pp)] = (pf[j] - nmean[S + u]) * ninv[S + u];
                }
            }
            for (int e = tid + MLP_TRAJ_PF * nthr; e < MLP_TP * U; e += nthr) {      // wide actions on few waves: fetched here
                const int pp = e / U, u = e - pp * U;
                const float v = (n0 + pp < B) ? q.seq[((size_t)(n0 + pp) * Hq + (t + 1)) * U + u] : 0.0f;
                act_n[e] = v;
                xs[tile_addr(S + u, pp)] = (v - nmean[S + u]) * ninv[S + u];
            }
        }
        __syncthreads();
        // ---- the step's outputs overlap the next step's first layer: the state tile row by row (S contiguous floats each),
        // the reward from wave 0, one lane per row.  `nxt` / `act_t` are next written behind step t + 1's Dense stack.
        if (q.states_out) {
            for (int i = tid; i < MLP_TP * S; i += nthr) {
                const int pp = i / S, s = i - pp * S;
                if (n0 + pp < B) q.states_out[((size_t)(n0 + pp) * Hq + t) * S + s] = nxt[pp * Sp + s];
            }
        }
        if (q.rewards_out && tid < MLP_TP && n0 + tid < B) {
            q.rewards_out[(size_t)(n0 + tid) * Hq + t] =
                reward_generic(q.reward_kind, q.fix_q1 != 0, cur + tid * Sp, act_t + tid * U, nxt + tid * Sp, S, U);
        }
    }
}

}  // namespace bbmpc
