// Trajectory distributions through the learned model (bbmpc_predict_trajectory_particles, kernels_traj_particles.hpp has
// the semantics, traj_particle_args.hpp the arguments): the frame of k_rollout_mlp_particles_kind
// (kernels_mlp_particles.hpp) -- 16 rows per workgroup, the generic MFMA recurrence of kernels_mlp.hpp (SPEC 0: v_mfma_f32_16x16x4_f32, packed wp4 operands, run-time activation
// codes), the state tile resident in LDS, the next step's actions and this step's noise in registers across the Dense
// stack, the member / head layers of kernels_mlp_ensemble.hpp / kernels_mlp_gaussian.hpp -- with three differences:
//   - rows are (b, p) pairs of a BATCH, each b with its own start state and action sequence: grid
//     (ceil(B * Pe / 16), 1, E), Pe = P / E; row r of member e = blockIdx.z is b = r / Pe, p = e + E * (r % Pe);
//   - after every step the row's S floats go to particle_states[((b * P + p) * Hq + t) * S ..] (row-contiguous, as
//     k_traj_mlp stores) and the step's reward to particle_rewards[(b * P + p) * Hq + t];
//   - no running sum, no NaN rule, no clip.
// One kernel text, k_traj_mlp_particles_kind<ARGS, EXT>, on one argument struct per kind as the rollout frame has them:
//   MlpTrajParticleArgs       k_traj_mlp_particles        one model (E = 1)
//   MlpEnsTrajParticleArgs    k_traj_mlp_particles_ens    a bootstrap ensemble with trajectory sampling
//   MlpGaussTrajParticleArgs  k_traj_mlp_particles_gauss  log-variance heads, with or without an ensemble
// Behind the LDS carve of mlp_traj_lds_layout / mlp_gauss_lds_layout lie 16 ints: per row of the tile the offset
// (b * P + p) * Hq of its rewards (times S: of its states), -1 for a row past the last -- the row map's divisions are
// done once, not per stored element.
// The prologue and the epilogue restate k_rollout_mlp_particles_kind / k_traj_mlp / rollout_mlp_body<0>: a fix in one of
// them belongs here as well.  Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_particles.hpp"
#include "traj_particle_args.hpp"

namespace bbmpc {

struct MlpTrajParticleArgs {
    static constexpr int KIND = MLP_PART_PLAIN;
    MlpDesc m;
    const float* wp4[MLP_MAX_LAYERS];    // MlpRolloutArgs::wp4
    int nw;                              // waves per workgroup
    TrajParticleArgs p;
};

struct MlpEnsTrajParticleArgs {
    static constexpr int KIND = MLP_PART_ENS;
    MlpDesc m;                           // as MlpEnsParticleArgs
    const float* wp4[MLP_MAX_LAYERS];
    int wstride[MLP_MAX_LAYERS];
    int bstride[MLP_MAX_LAYERS];
    int nw;
    int E;
    TrajParticleArgs p;
};

struct MlpGaussTrajParticleArgs {
    static constexpr int KIND = MLP_PART_GAUSS;
    MlpDesc m;                           // as MlpGaussParticleArgs
    const float* wp4[MLP_MAX_LAYERS];
    int wstride[MLP_MAX_LAYERS];
    int bstride[MLP_MAX_LAYERS];
    const float* hp4;
    const float* hbp;
    int hwstride, hbstride;
    const float* min_logvar;
    const float* max_logvar;
    int nw;
    int E;
    TrajParticleArgs p;
};

constexpr int MLP_TRAJ_PART_ROWMAP = MLP_TP;      // ints behind the layout's total

template <class ARGS, bool EXT>
__global__ void k_traj_mlp_particles_kind(ARGS q) {
    constexpr int KIND = ARGS::KIND;
    constexpr bool MEMBER = KIND != MLP_PART_PLAIN;       // rows grouped by member, grid.z = member
    constexpr bool GAUSS = KIND == MLP_PART_GAUSS;        // a log-variance head behind the last layer
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& m = q.m;
    const TrajParticleArgs& pa = q.p;
    const int e = MEMBER ? (int)blockIdx.z : 0;           // the member of every row of this workgroup
    const int n0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = pa.S, U = pa.U, Hq = pa.Hq, L = m.n_layers, P = pa.P;
    int E = 1, Pe = P;                          // members, particles per member
    if constexpr (MEMBER) {
        E = q.E;
        Pe = P / E;
    }
    const int R = pa.B * Pe;                    // rows of this member
    const int Sp = (S + 3) & ~3;
    const MlpTrajLds lay = GAUSS ? mlp_gauss_lds_layout(m, U, S, nw) : mlp_traj_lds_layout(m, U, S, nw);
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
    float* hbias = lbias + S;                   // GAUSS: [S] bias of the log-variance head
    float* minlv = hbias + S;                   // GAUSS: [S] bounds of the soft clamp
    float* maxlv = minlv + S;
    int* rowoff = reinterpret_cast<int*>(smem + lay.total);       // [16] (b * P + p) * Hq of the tile's rows, -1 = none

    // ---- the row map: row r of this member -> batch row, particle
    auto row_b = [&](int r) -> int { return r / Pe; };
    auto row_p = [&](int r) -> int {
        if constexpr (MEMBER) return e + E * (r % Pe);
        else return r % Pe;
    };
    // ---- the operands and packed biases of layer l
    auto layer_w = [&](int l) -> const float* {
        if constexpr (MEMBER) return q.wp4[l] + e * q.wstride[l];
        else return q.wp4[l];
    };
    auto layer_b = [&](int l) -> const float* {
        if constexpr (MEMBER) return m.bpack[l] + e * q.bstride[l];
        else return m.bpack[l];
    };
    // ---- what a fetched noise element is: sigma[f] * eps, or eps alone where the scale is known only behind the Dense stack
    auto noise_elem = [&](float sig, float eps) -> float {
        if constexpr (GAUSS) return eps;
        else return sig * eps;
    };

    // what this thread fetches every step, fixed across the horizon: action elements el = tid + j * nthr of the tile
    // [16][U] (offset of step 0 in seq, -1 = none; U floats between steps) and noise elements i = tid + j * nthr of the
    // tile [S][16] (offset of step 0 in eps, -1 = a row past the last).  32-bit offsets: the host refuses larger buffers.
    int abase[MLP_TRAJ_PF];
#pragma unroll
    for (int j = 0; j < MLP_TRAJ_PF; ++j) {
        const int el = tid + j * nthr;
        const int pp = el / U, u = el - pp * U;
        abase[j] = -1;
        if (el < MLP_TP * U && n0 + pp < R) abase[j] = row_b(n0 + pp) * Hq * U + u;
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
            nbase[j] = (row_b(n0 + pp) * P + row_p(n0 + pp)) * Hq * S + f;
            nsig[j] = pa.sigma[f];
        }
    }
    // the same elements without the registers (wide tiles on few waves)
    auto fetch_action = [&](int el, int t) -> float {
        const int pp = el / U, u = el - pp * U;
        if (n0 + pp >= R) return 0.0f;
        return pa.seq[((size_t)row_b(n0 + pp) * Hq + t) * U + u];
    };
    auto fetch_noise = [&](int i, int t) -> float {
        const int f = i / MLP_TP, pp = i - f * MLP_TP;
        if (n0 + pp >= R) return 0.0f;
        return noise_elem(pa.sigma[f], pa.eps[(((size_t)row_b(n0 + pp) * P + row_p(n0 + pp)) * Hq + t) * S + f]);
    };

    if (tid < MLP_TP) rowoff[tid] = (n0 + tid < R) ? (row_b(n0 + tid) * P + row_p(n0 + tid)) * Hq : -1;
    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? m.mean_s[f] : m.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? m.std_s[f] : m.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;          // system_dynamics_handler.py:119-122 (x - mu)/(sd + 1e-7)
        if (f < S) {
            tmean[f] = normd ? m.mean_t[f] : 0.0f;
            tstd[f] = normd ? (m.std_t[f] + 1e-7f) : 1.0f;
            const size_t bslot = ((size_t)(f >> 4) * 64 + ((f & 15) >> 2) * 16) * 4 + (f & 3);     // feature f in [OT][64][4]
            lbias[f] = layer_b(L - 1)[bslot];
            if constexpr (GAUSS) {
                hbias[f] = (q.hbp + e * q.hbstride)[bslot];
                minlv[f] = q.min_logvar[f];
                maxlv[f] = q.max_logvar[f];
            }
        }
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) xs[i] = 0.0f;
    for (int i = tid; i < MLP_TP * S; i += nthr) {                 // every row starts from its batch row's state
        const int pp = i / S, s = i % S;
        st[pp * Sp + s] = (n0 + pp < R) ? pa.states[(size_t)row_b(n0 + pp) * S + s] : 0.0f;
    }
    for (int el = tid; el < MLP_TP * U; el += nthr) acts[el] = fetch_action(el, 0);     // (rows past the last roll zeros)
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
        // ---- in flight across the Dense stack: the next step's action elements and this step's noise elements
        float pf[MLP_TRAJ_PF];
#pragma unroll
        for (int j = 0; j < MLP_TRAJ_PF; ++j) pf[j] = (more && abase[j] >= 0) ? pa.seq[abase[j] + (t + 1) * U] : 0.0f;
        float en[MLP_PART_PF];
#pragma unroll
        for (int j = 0; j < MLP_PART_PF; ++j) en[j] = nbase[j] >= 0 ? noise_elem(nsig[j], pa.eps[nbase[j] + t * S]) : 0.0f;
        // ---- dense layers (kernels_mlp.hpp, SPEC 0)
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            if constexpr (MEMBER) mlp_layer_out_split_member<EXT>(m, layer_w(l), layer_b(l), l, in_off, out_off, wave, lane, nw);
            else mlp_layer_out_split<EXT>(m, layer_w(l), l, in_off, out_off, wave, lane, nw);
            __syncthreads();
            in_off = out_off;
        }
        if constexpr (GAUSS) mlp_layer_k_split_gauss(m, layer_w(L - 1), q.hp4 + e * q.hwstride, L - 1, in_off, lay.part, wave, lane, nw);
        else mlp_layer_k_split(m, layer_w(L - 1), L - 1, in_off, lay.part, wave, lane, nw);
        __syncthreads();
        // ---- epilogue: reduce partials (GAUSS: the head's too), bias, last activation (mean only), de-normalise, residual,
        // NOISE (GAUSS: scaled here); stage step t + 1's input.  `d` is a noise_elem, `sig` its sigma[f] (read by GAUSS only).
        const int nwp = min(nw, m.tiles[L - 1]);          // waves that actually produced partials
        auto epilogue = [&](int i, float sig, float d) {
            const int f = i / MLP_TP, pp = i % MLP_TP;
            const int ot = f >> 4, ln = ((f & 15) >> 2) * 16 + pp, rg = f & 3;
            const float* pp0 = part + (((size_t)ot) * 64 + ln) * 4 + rg;
            [[maybe_unused]] const float* hp0 = pp0 + (size_t)nw * OTl * 256;       // GAUSS: the head's partials lie behind the mean's
            float acc = lbias[f];
            for (int w = 0; w < nwp; ++w) acc = acc + pp0[(size_t)w * OTl * 256];
            float z = 0.0f;
            if constexpr (GAUSS) {
                z = hbias[f];
                for (int w = 0; w < nwp; ++w) z = z + hp0[(size_t)w * OTl * 256];
            }
            acc = apply_act_rt<EXT>(acc, m.act[L - 1]);                     // (the head has no activation)
            const float dev = normd ? tmean[f] + acc * tstd[f] : acc;       // system_dynamics_handler.py:152-155
            if constexpr (GAUSS) {
                const float lv1 = maxlv[f] - bb_softplusf(maxlv[f] - z);    // PETS' soft clamp of the log-variance
                const float lv = minlv[f] + bb_softplusf(lv1 - minlv[f]);
                const float sd = tstd[f] * bb_exp_rel(0.5f * lv);           // (tstd is 1 when not normalised)
                d = (sig + sd) * d;
            }
            const float ns = (dev + cur[pp * Sp + f]) + d;                  // transforms.py:34, + sigma * eps / (sigma + sd) * eps
            nxt[pp * Sp + f] = ns;
            xs[tile_addr(f, pp)] = (ns - nmean[f]) * ninv[f];
        };
#pragma unroll
        for (int j = 0; j < MLP_PART_PF; ++j) {
            const int i = tid + j * nthr;
            if (i < MLP_TP * S) epilogue(i, nsig[j], en[j]);
        }
        for (int i = tid + MLP_PART_PF * nthr; i < MLP_TP * S; i += nthr) epilogue(i, pa.sigma[i / MLP_TP], fetch_noise(i, t));
        if (more) {
#pragma unroll
            for (int j = 0; j < MLP_TRAJ_PF; ++j) {
                const int el = tid + j * nthr;
                if (el < MLP_TP * U) {
                    const int pp = el / U, u = el - pp * U;
                    act_n[el] = pf[j];
                    xs[tile_addr(S + u, pp)] = (pf[j] - nmean[S + u]) * ninv[S + u];
                }
            }
            for (int el = tid + MLP_TRAJ_PF * nthr; el < MLP_TP * U; el += nthr) {      // wide actions on few waves: fetched here
                const int pp = el / U, u = el - pp * U;
                const float v = fetch_action(el, t + 1);
                act_n[el] = v;
                xs[tile_addr(S + u, pp)] = (v - nmean[S + u]) * ninv[S + u];
            }
        }
        __syncthreads();
        // ---- the step's outputs overlap the next step's first layer: the state tile row by row (S contiguous floats each),
        // the reward from wave 0, one lane per row.  `nxt` / `cur` / `act_t` are next written behind step t + 1's Dense stack,
        // whose barriers every wave passes after this.
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int pp = i / S, s = i - pp * S;
            const int ro = rowoff[pp];
            if (ro >= 0) pa.pstates[(ro + t) * S + s] = nxt[pp * Sp + s];
        }
        if (tid < MLP_TP && rowoff[tid] >= 0)
            pa.prewards[rowoff[tid] + t] = reward_generic(pa.reward_kind, pa.fix_q1 != 0, cur + tid * Sp, act_t + tid * U, nxt + tid * Sp, S, U);
    }
}

}  // namespace bbmpc
