// Particle rollouts through the learned model (kernels_particles.hpp has the semantics): the frame of k_traj_mlp
// (kernels_mlp_traj.hpp) -- 16 rows per workgroup, the generic MFMA recurrence of kernels_mlp.hpp (SPEC 0:
// v_mfma_f32_16x16x4_f32, packed wp4 operands, run-time activation codes), the state tile resident in LDS, the next step's
// actions fetched while the Dense stack runs -- with rows that are (candidate, particle) pairs of ONE agent
// (grid.y = agent, row = n * P + p, so a tile mixes candidates and two rows share an action only when they share n):
//   - every row starts from the agent's state;
//   - the step's noise elements sigma[f] * eps[a, p, t, f] are fetched in front of the Dense stack, held in registers
//     across it and added in the epilogue, so the noisy state is what the reward and the next step see;
//   - the reward is summed per row in a register of wave 0's first 16 lanes; nothing is stored per step, the NaN rule and
//     one store per row close the kernel.
// The prologue and the epilogue restate k_traj_mlp / rollout_mlp_body<0>: a fix in one of them belongs here as well.
// Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_traj.hpp"
#include "kernels_particles.hpp"

namespace bbmpc {

struct MlpParticleArgs {
    MlpDesc m;
    const float* wp4[MLP_MAX_LAYERS];    // MlpRolloutArgs::wp4
    int nw;                              // waves per workgroup
    ParticleArgs p;
};

constexpr int MLP_PART_PF = 2;      // noise elements a thread holds in registers across a step's Dense stack

template <bool EXT>
__global__ void k_rollout_mlp_particles(MlpParticleArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& m = q.m;
    const ParticleArgs& pa = q.p;
    const int a = blockIdx.y;
    const int n0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = pa.S, U = pa.U, H = pa.H, L = m.n_layers, P = pa.P;
    const int R = pa.n_pop * P;                    // rows of this agent
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

    // what this thread fetches every step, fixed across the horizon: action elements e = tid + j * nthr of the tile
    // [16][U] (offset of step 0 and the distance between steps, -1 = none) and noise elements i = tid + j * nthr of the
    // tile [S][16] (offset of step 0 in pnoise, -1 = a row past the agent's).  32-bit offsets: the host refuses larger buffers.
    const float* asrc = pa.from_ref ? pa.seq : pa.cand;
    const int act_step = pa.from_ref ? U : U * pa.Nst;
    int abase[MLP_TRAJ_PF];
#pragma unroll
    for (int j = 0; j < MLP_TRAJ_PF; ++j) {
        const int e = tid + j * nthr;
        const int pp = e / U, u = e - pp * U;
        abase[j] = -1;
        if (e < MLP_TP * U && n0 + pp < R) {
            const int n = (n0 + pp) / P;
            abase[j] = pa.from_ref ? (n * pa.A + a) * pa.HU + u : (a * pa.HU + u) * pa.Nst + n;
        }
    }
    int nbase[MLP_PART_PF];
    float nsig[MLP_PART_PF];
#pragma unroll
    for (int j = 0; j < MLP_PART_PF; ++j) {
        const int i = tid + j * nthr;
        const int f = i / MLP_TP, pp = i - f * MLP_TP;
        nbase[j] = -1;
        nsig[j] = 0.0f;
        if (i < MLP_TP * S && n0 + pp < R) {
            const int p = (n0 + pp) % P;
            nbase[j] = (a * P + p) * H * S + f;
            nsig[j] = pa.sigma[f];
        }
    }
    // the same elements without the registers (wide tiles on few waves)
    auto fetch_action = [&](int e, int t) -> float {
        const int pp = e / U, u = e - pp * U;
        if (n0 + pp >= R) return 0.0f;
        return particle_action(pa, a, (n0 + pp) / P, t, u);
    };
    auto fetch_noise = [&](int i, int t) -> float {
        const int f = i / MLP_TP, pp = i - f * MLP_TP;
        if (n0 + pp >= R) return 0.0f;
        return pa.sigma[f] * pa.pnoise[(((size_t)a * P + (n0 + pp) % P) * H + t) * S + f];
    };

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
    for (int i = tid; i < MLP_TP * S; i += nthr) {                 // tf.tile(current_states, ...): every row, the agent's state
        const int pp = i / S, s = i % S;
        st[pp * Sp + s] = pa.state[(size_t)a * S + s];
    }
    for (int e = tid; e < MLP_TP * U; e += nthr) acts[e] = fetch_action(e, 0);     // (rows past the agent's roll zeros)
    __syncthreads();
    for (int i = tid; i < MLP_TP * (S + U); i += nthr) {          // normalised layer-0 input for t = 0
        const int f = i / MLP_TP, pp = i % MLP_TP;
        const float v = (f < S) ? st[pp * Sp + f] : acts[pp * U + (f - S)];
        xs[tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
    }
    __syncthreads();

    const int OTl = m.tiles[L];
    float racc = 0.0f;                                 // lanes 0..15 of wave 0: the row's reward sum
    for (int t = 0; t < H; ++t) {
        float* cur = st + (t & 1) * MLP_TP * Sp;
        float* nxt = st + ((t + 1) & 1) * MLP_TP * Sp;
        const float* act_t = acts + (t & 1) * MLP_TP * U;
        float* act_n = acts + ((t + 1) & 1) * MLP_TP * U;
        const bool more = t + 1 < H;
        // ---- in flight across the Dense stack: the next step's action elements and this step's noise elements
        float pf[MLP_TRAJ_PF];
#pragma unroll
        for (int j = 0; j < MLP_TRAJ_PF; ++j) {
            float v = 0.0f;
            if (more && abase[j] >= 0) {
                v = asrc[abase[j] + (t + 1) * act_step];
                if (pa.pen) {
                    const int u = (tid + j * nthr) % U;
                    v = clipf(v, pa.lo[u], pa.hi[u]);
                }
            }
            pf[j] = v;
        }
        float en[MLP_PART_PF];
#pragma unroll
        for (int j = 0; j < MLP_PART_PF; ++j) en[j] = nbase[j] >= 0 ? nsig[j] * pa.pnoise[nbase[j] + t * S] : 0.0f;
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
        // ---- epilogue: reduce partials, bias, last activation, de-normalise, residual, NOISE; stage step t + 1's input
        const int nwp = min(nw, m.tiles[L - 1]);          // waves that actually produced partials
        auto epilogue = [&](int i, float d) {
            const int f = i / MLP_TP, pp = i % MLP_TP;
            const int ot = f >> 4, ln = ((f & 15) >> 2) * 16 + pp, rg = f & 3;
            const float* pp0 = part + (((size_t)ot) * 64 + ln) * 4 + rg;
            float acc = lbias[f];
            for (int w = 0; w < nwp; ++w) acc = acc + pp0[(size_t)w * OTl * 256];
            acc = apply_act_rt<EXT>(acc, m.act[L - 1]);
            const float dev = normd ? tmean[f] + acc * tstd[f] : acc;       // system_dynamics_handler.py:152-155
            const float ns = (dev + cur[pp * Sp + f]) + d;                  // transforms.py:34, + sigma * eps
            nxt[pp * Sp + f] = ns;
            xs[tile_addr(f, pp)] = (ns - nmean[f]) * ninv[f];
        };
#pragma unroll
        for (int j = 0; j < MLP_PART_PF; ++j) {
            const int i = tid + j * nthr;
            if (i < MLP_TP * S) epilogue(i, en[j]);
        }
        for (int i = tid + MLP_PART_PF * nthr; i < MLP_TP * S; i += nthr) epilogue(i, fetch_noise(i, t));
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
                const float v = fetch_action(e, t + 1);
                act_n[e] = v;
                xs[tile_addr(S + u, pp)] = (v - nmean[S + u]) * ninv[S + u];
            }
        }
        __syncthreads();
        // ---- the step's reward overlaps the next step's first layer: wave 0, one lane per row.  `cur` / `act_t` are next
        // written behind step t + 1's Dense stack, whose barriers wave 0 passes after this.
        if (tid < MLP_TP)
            racc = racc + reward_generic(pa.reward_kind, pa.fix_q1 != 0, cur + tid * Sp, act_t + tid * U, nxt + tid * Sp, S, U);
    }
    if (tid < MLP_TP && n0 + tid < R) {
        if (racc != racc) racc = -1.0e6f;                       // deterministic.py:75-77, per particle
        pa.returns[(size_t)a * pa.RS + n0 + tid] = racc;
    }
}

}  // namespace bbmpc
