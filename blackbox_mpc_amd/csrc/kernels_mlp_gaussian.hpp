// Particle rollouts through PROBABILISTIC learned models (bbmpc_set_mlp_logvar_head): every model --
// the handle's, or each member of its ensemble -- carries a log-variance head, a second last Dense layer on the last hidden
// activation, and the noise scale of a step becomes state dependent:
//     nxt = predict_next_state_member(s_t, a_t) + (sigma[f] + sd_f(s_t, a_t)) * eps[a, p, t, f]
//     z = h W_v + b_v;  lv1 = max_lv - softplus(max_lv - z);  lv = min_lv + softplus(lv1 - min_lv);  sd = tstd * exp(lv / 2)
// The frame is k_rollout_mlp_particles_ens' (kernels_mlp_ensemble.hpp): grid (ceil(n_pop * Pe / 16), A, E), the same
// row -> (candidate, particle) map, hidden layers through mlp_layer_out_split_member.  Without an ensemble E = 1 with the
// primary's operands and stride 0, and the map is k_rollout_mlp_particles': one kernel serves both.
// The last layer multiplies the input tile into the mean's output tiles and into the head's (packed by mlp_pack_layer like
// the mean's, [OT][IT][64][4] per member): two independent accumulator chains per k tile, the mean's in the order
// mlp_layer_k_split runs them, so the mean has the bits the ensemble kernel gives.  The head's partial sums lie behind the
// mean's in LDS (mlp_gauss_lds_layout: `part` doubled, three more [S] vectors in `norm`).
// The noise registers hold eps, not sigma * eps: the scale is known only behind the Dense stack.
// The prologue and the epilogue restate k_rollout_mlp_particles_ens: a fix in one of them belongs here as well.
// Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_ensemble.hpp"

namespace bbmpc {

constexpr float MLP_LOGVAR_ABS_MAX = 40.0f;      // |min_logvar|, |max_logvar| <= 40: exp(lv / 2) stays far inside fp32

struct MlpGaussParticleArgs {
    MlpDesc m;                           // the primary's dims / activations / statistics; bpack = member 0's packed biases
    const float* wp4[MLP_MAX_LAYERS];    // member 0's packed operands (MlpRolloutArgs::wp4's layout)
    int wstride[MLP_MAX_LAYERS];         // floats between two members' operands of a layer (0 without an ensemble)
    int bstride[MLP_MAX_LAYERS];         // ... and between their packed biases
    const float* hp4;                    // head 0's packed operands, the last layer's layout [OT][IT][64][4]
    const float* hbp;                    // head 0's packed biases [OT][64][4]
    int hwstride, hbstride;              // floats between two heads
    const float* min_logvar;             // [S]
    const float* max_logvar;             // [S]
    int nw;                              // waves per workgroup
    int E;                               // members (1 without an ensemble)
    ParticleArgs p;
};

// mlp_traj_lds_layout with room for the head: `part` [2][NW][OTlast][64][4], `norm` + (head bias, min_lv, max_lv) [S] each
__host__ __device__ inline MlpTrajLds mlp_gauss_lds_layout(const MlpDesc& m, int U, int S, int nw) {
    MlpTrajLds l;
    int itmax = 1;
    for (int i = 1; i < m.n_layers; ++i) itmax = itmax > m.tiles[i] ? itmax : m.tiles[i];
    const int Sp = (S + 3) & ~3;
    int o = 0;
    l.xs = o;   o += m.tiles[0] * 256;
    l.actA = o; o += itmax * 256;
    l.actB = o; o += itmax * 256;
    l.part = o; o += 2 * nw * m.tiles[m.n_layers] * 256;
    l.st = o;   o += 2 * MLP_TP * Sp;
    l.acts = o; o += ((2 * MLP_TP * U + 3) & ~3);
    l.norm = o; o += (((S + U) * 2 + S * 6 + 63) & ~63);
    l.total = o;
    return l;
}

// Last layer and head, K split (mlp_layer_k_split, kernels_mlp.hpp): a wave multiplies the input tiles it owns into every
// output tile of the mean and of the head and leaves part[wave][ot][lane] and, nw * OT tiles behind it, the head's.
__device__ __forceinline__ void mlp_layer_k_split_gauss(const MlpDesc& m, const float* wp4, const float* hp4, int l, int in_off,
                                                        int part_off, int wave, int lane, int nw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];        // (offsets, not pointers: see mlp_layer_out_split)
    const float* in = smem + in_off;
    float* part = smem + part_off;
    const int IT = m.tiles[l], OT = m.tiles[l + 1];
    const f32x4* __restrict__ W = reinterpret_cast<const f32x4*>(wp4);
    const f32x4* __restrict__ V = reinterpret_cast<const f32x4*>(hp4);
    for (int ot = 0; ot < OT; ++ot) {
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        f32x4 hacc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int it = wave; it < IT; it += nw) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(in + ((size_t)it * 64 + lane) * 4);
            const f32x4 w = W[((size_t)ot * IT + it) * 64 + lane];
            const f32x4 v = V[((size_t)ot * IT + it) * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b.x, acc, 0, 0, 0);
            hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, b.x, hacc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b.y, acc, 0, 0, 0);
            hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, b.y, hacc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, b.z, acc, 0, 0, 0);
            hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, b.z, hacc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, b.w, acc, 0, 0, 0);
            hacc = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, b.w, hacc, 0, 0, 0);
        }
        *reinterpret_cast<f32x4*>(part + (((size_t)wave * OT + ot) * 64 + lane) * 4) = acc;
        *reinterpret_cast<f32x4*>(part + (((size_t)(nw + wave) * OT + ot) * 64 + lane) * 4) = hacc;
    }
}

template <bool EXT>
__global__ void k_rollout_mlp_particles_gauss(MlpGaussParticleArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& m = q.m;
    const ParticleArgs& pa = q.p;
    const int a = blockIdx.y;
    const int e = blockIdx.z;                         // the member of every row of this workgroup
    const int n0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = pa.S, U = pa.U, H = pa.H, L = m.n_layers, P = pa.P, E = q.E;
    const int Pe = P / E;                             // particles per member
    const int R = pa.n_pop * Pe;                      // rows of this (agent, member)
    const int Sp = (S + 3) & ~3;
    const MlpTrajLds lay = mlp_gauss_lds_layout(m, U, S, nw);
    float* xs = smem + lay.xs;
    float* part = smem + lay.part;
    float* st = smem + lay.st;
    float* acts = smem + lay.acts;
    const bool normd = m.normalized != 0;
    float* nmean = smem + lay.norm;             // [S+U] input means (0 when not normalised)
    float* ninv = nmean + (S + U);              // [S+U] 1/(std + 1e-7)   (1 when not normalised)
    float* tmean = ninv + (S + U);              // [S] target mean
    float* tstd = tmean + S;                    // [S] target std + 1e-7
    float* lbias = tstd + S;                    // [S] bias of the member's last layer
    float* hbias = lbias + S;                   // [S] bias of the member's log-variance head
    float* minlv = hbias + S;                   // [S] bounds of the soft clamp
    float* maxlv = minlv + S;

    // row r -> (candidate, particle): the rows of a member walk its particles e, e + E, ... of candidate 0, then candidate 1's
    auto row_n = [&](int r) -> int { return r / Pe; };
    auto row_p = [&](int r) -> int { return e + E * (r % Pe); };

    // what this thread fetches every step, fixed across the horizon (k_rollout_mlp_particles): action elements of the tile
    // [16][U] and noise elements of the tile [S][16], 32-bit offsets, -1 = none
    const float* asrc = pa.from_ref ? pa.seq : pa.cand;
    const int act_step = pa.from_ref ? U : U * pa.Nst;
    int abase[MLP_TRAJ_PF];
#pragma unroll
    for (int j = 0; j < MLP_TRAJ_PF; ++j) {
        const int el = tid + j * nthr;
        const int pp = el / U, u = el - pp * U;
        abase[j] = -1;
        if (el < MLP_TP * U && n0 + pp < R) {
            const int n = row_n(n0 + pp);
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
            nbase[j] = (a * P + row_p(n0 + pp)) * H * S + f;
            nsig[j] = pa.sigma[f];
        }
    }
    // the same elements without the registers (wide tiles on few waves)
    auto fetch_action = [&](int el, int t) -> float {
        const int pp = el / U, u = el - pp * U;
        if (n0 + pp >= R) return 0.0f;
        return particle_action(pa, a, row_n(n0 + pp), t, u);
    };
    auto fetch_noise = [&](int i, int t) -> float {
        const int f = i / MLP_TP, pp = i - f * MLP_TP;
        if (n0 + pp >= R) return 0.0f;
        return pa.pnoise[(((size_t)a * P + row_p(n0 + pp)) * H + t) * S + f];
    };

    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? m.mean_s[f] : m.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? m.std_s[f] : m.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;          // system_dynamics_handler.py:119-122 (x - mu)/(sd + 1e-7)
        if (f < S) {
            tmean[f] = normd ? m.mean_t[f] : 0.0f;
            tstd[f] = normd ? (m.std_t[f] + 1e-7f) : 1.0f;
            const size_t bslot = ((size_t)(f >> 4) * 64 + ((f & 15) >> 2) * 16) * 4 + (f & 3);     // feature f in [OT][64][4]
            lbias[f] = (m.bpack[L - 1] + e * q.bstride[L - 1])[bslot];
            hbias[f] = (q.hbp + e * q.hbstride)[bslot];
            minlv[f] = q.min_logvar[f];
            maxlv[f] = q.max_logvar[f];
        }
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) xs[i] = 0.0f;
    for (int i = tid; i < MLP_TP * S; i += nthr) {                 // every row, the agent's state
        const int pp = i / S, s = i % S;
        st[pp * Sp + s] = pa.state[(size_t)a * S + s];
    }
    for (int el = tid; el < MLP_TP * U; el += nthr) acts[el] = fetch_action(el, 0);     // (rows past the member's roll zeros)
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
        for (int j = 0; j < MLP_PART_PF; ++j) en[j] = nbase[j] >= 0 ? pa.pnoise[nbase[j] + t * S] : 0.0f;        // eps, not sigma * eps
        // ---- dense layers (kernels_mlp.hpp, SPEC 0) on member e's operands
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            mlp_layer_out_split_member<EXT>(m, q.wp4[l] + e * q.wstride[l], m.bpack[l] + e * q.bstride[l], l, in_off, out_off, wave, lane, nw);
            __syncthreads();
            in_off = out_off;
        }
        mlp_layer_k_split_gauss(m, q.wp4[L - 1] + e * q.wstride[L - 1], q.hp4 + e * q.hwstride, L - 1, in_off, lay.part, wave, lane, nw);
        __syncthreads();
        // ---- epilogue: reduce both partials, biases, last activation (mean only), de-normalise, residual, sd, NOISE; stage step t + 1's input
        const int nwp = min(nw, m.tiles[L - 1]);          // waves that actually produced partials
        auto epilogue = [&](int i, float sig, float eps) {
            const int f = i / MLP_TP, pp = i % MLP_TP;
            const int ot = f >> 4, ln = ((f & 15) >> 2) * 16 + pp, rg = f & 3;
            const float* pp0 = part + (((size_t)ot) * 64 + ln) * 4 + rg;
            const float* hp0 = pp0 + (size_t)nw * OTl * 256;                // the head's partials lie behind the mean's
            float acc = lbias[f];
            for (int w = 0; w < nwp; ++w) acc = acc + pp0[(size_t)w * OTl * 256];
            float z = hbias[f];
            for (int w = 0; w < nwp; ++w) z = z + hp0[(size_t)w * OTl * 256];
            acc = apply_act_rt<EXT>(acc, m.act[L - 1]);                     // (the head has no activation)
            const float dev = normd ? tmean[f] + acc * tstd[f] : acc;       // system_dynamics_handler.py:152-155
            const float lv1 = maxlv[f] - bb_softplusf(maxlv[f] - z);        // PETS' soft clamp of the log-variance
            const float lv = minlv[f] + bb_softplusf(lv1 - minlv[f]);
            const float sd = tstd[f] * bb_exp_rel(0.5f * lv);               // (tstd is 1 when not normalised)
            const float d = (sig + sd) * eps;
            const float ns = (dev + cur[pp * Sp + f]) + d;                  // transforms.py:34, + (sigma + sd) * eps
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
        // ---- the step's reward overlaps the next step's first layer: wave 0, one lane per row.  `cur` / `act_t` are next
        // written behind step t + 1's Dense stack, whose barriers wave 0 passes after this.
        if (tid < MLP_TP)
            racc = racc + reward_generic(pa.reward_kind, pa.fix_q1 != 0, cur + tid * Sp, act_t + tid * U, nxt + tid * Sp, S, U);
    }
    if (tid < MLP_TP && n0 + tid < R) {
        if (racc != racc) racc = -1.0e6f;                       // deterministic.py:75-77, per particle
        pa.returns[(size_t)a * pa.RS + (size_t)row_n(n0 + tid) * P + row_p(n0 + tid)] = racc;
    }
}

}  // namespace bbmpc
