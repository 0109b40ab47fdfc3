// Particle rollouts through a bootstrap ENSEMBLE of learned models (bbmpc_set_mlp_ensemble):
// trajectory sampling, particle p of every candidate follows member p % E for the whole horizon.  The frame is
// k_rollout_mlp_particles' (kernels_mlp_particles.hpp) -- 16 rows per workgroup, v_mfma_f32_16x16x4_f32 on the packed wp4
// operands, the state tile resident in LDS, LDS addressed by offsets, the next step's actions and this step's noise in
// registers across the Dense stack, the reward summed in wave 0's first 16 lanes, one store per row -- over another row
// space: an MFMA tile multiplies ONE set of weights, so a tile must be uniform in the member.
//     grid (ceil(n_pop * Pe / 16), A, E),  Pe = P / E        (the host refuses P % E != 0)
//     row r of member e = blockIdx.z:  candidate n = r / Pe,  particle p = e + E * (r % Pe),  store returns[a * RS + n * P + p]
// The members' packed operands [OT][IT][64][4] and biases [OT][64][4] of a layer lie one behind the other at a fixed
// stride: the kernel adds e * stride to the base pointers, uniform per workgroup (scalar registers, no pointer table).
// Dims, activations and the normalisation statistics are the primary model's (MlpDesc).  The LDS layout is
// mlp_traj_lds_layout, offsets are 32 bit as in k_rollout_mlp_particles (the host refuses larger buffers).
// The prologue and the epilogue restate k_rollout_mlp_particles: a fix in one of them belongs here as well.
// Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_particles.hpp"

namespace bbmpc {

constexpr int MLP_ENS_MAX = 8;           // members of an ensemble

struct MlpEnsParticleArgs {
    MlpDesc m;                           // the primary's dims / activations / statistics; bpack = member 0's packed biases
    const float* wp4[MLP_MAX_LAYERS];    // member 0's packed operands (MlpRolloutArgs::wp4's layout)
    int wstride[MLP_MAX_LAYERS];         // floats between two members' operands of a layer
    int bstride[MLP_MAX_LAYERS];         // ... and between their packed biases
    int nw;                              // waves per workgroup
    int E;                               // members
    ParticleArgs p;
};

// mlp_layer_out_split (kernels_mlp.hpp; the measurements behind its shape are written there) with the layer's packed biases
// passed in, where that one reads m.bpack[l]: the member's, at the same [OT][64][4] layout.  Statement for statement the
// same arithmetic, so a member equal to the primary gives the primary's bits.
template <bool EXT>
__device__ __forceinline__ void mlp_layer_out_split_member(const MlpDesc& m, const float* wp4, const float* bias, int l, int in_off,
                                                           int out_off, int wave, int lane, int nw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const float* in = smem + in_off;
    float* out = smem + out_off;
    const int IT = m.tiles[l], OT = m.tiles[l + 1];
    const f32x4* __restrict__ W = reinterpret_cast<const f32x4*>(wp4);
    const float* __restrict__ bp = bias;
    const int a = m.act[l];
    for (int ot0 = wave; ot0 < OT; ot0 += 2 * nw) {
        const int ot1 = ot0 + nw;
        if (ot1 < OT) {
            f32x4 acc0 = *reinterpret_cast<const f32x4*>(bp + ((size_t)ot0 * 64 + lane) * 4);
            f32x4 acc1 = *reinterpret_cast<const f32x4*>(bp + ((size_t)ot1 * 64 + lane) * 4);
            const f32x4* w0 = W + (size_t)ot0 * IT * 64 + lane;
            const f32x4* w1 = W + (size_t)ot1 * IT * 64 + lane;
            f32x4 r0[MLP_GEN_PF], r1[MLP_GEN_PF];
#pragma unroll
            for (int j = 0; j < MLP_GEN_PF; ++j) {
                const int kk = j < IT ? j : IT - 1;
                r0[j] = w0[(size_t)kk * 64];
                r1[j] = w1[(size_t)kk * 64];
            }
            for (int it = 0; it < IT; it += MLP_GEN_PF) {
#pragma unroll
                for (int j = 0; j < MLP_GEN_PF; ++j) {
                    const int k = it + j;
                    if (k < IT) {
                        const f32x4 b = *reinterpret_cast<const f32x4*>(in + ((size_t)k * 64 + lane) * 4);
                        const f32x4 a0 = r0[j], a1 = r1[j];
                        const int kn = k + MLP_GEN_PF < IT ? k + MLP_GEN_PF : IT - 1;
                        r0[j] = w0[(size_t)kn * 64];
                        r1[j] = w1[(size_t)kn * 64];
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b.x, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.x, b.x, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b.y, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.y, b.y, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b.z, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.z, b.z, acc1, 0, 0, 0);
                        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b.w, acc0, 0, 0, 0);
                        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1.w, b.w, acc1, 0, 0, 0);
                    }
                }
            }
            acc0 = apply_act4<EXT>(acc0, a);
            acc1 = apply_act4<EXT>(acc1, a);
            *reinterpret_cast<f32x4*>(out + ((size_t)ot0 * 64 + lane) * 4) = acc0;
            *reinterpret_cast<f32x4*>(out + ((size_t)ot1 * 64 + lane) * 4) = acc1;
        } else {
            f32x4 acc = *reinterpret_cast<const f32x4*>(bp + ((size_t)ot0 * 64 + lane) * 4);
            const f32x4* w0 = W + (size_t)ot0 * IT * 64 + lane;
#pragma unroll 4
            for (int it = 0; it < IT; ++it) {
                const f32x4 b = *reinterpret_cast<const f32x4*>(in + ((size_t)it * 64 + lane) * 4);
                const f32x4 a0 = w0[(size_t)it * 64];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b.w, acc, 0, 0, 0);
            }
            acc = apply_act4<EXT>(acc, a);
            *reinterpret_cast<f32x4*>(out + ((size_t)ot0 * 64 + lane) * 4) = acc;
        }
    }
}

template <bool EXT>
__global__ void k_rollout_mlp_particles_ens(MlpEnsParticleArgs q) {
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
    float* lbias = tstd + S;                    // [S] bias of the member's last layer

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
        return pa.sigma[f] * pa.pnoise[(((size_t)a * P + row_p(n0 + pp)) * H + t) * S + f];
    };

    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? m.mean_s[f] : m.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? m.std_s[f] : m.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;          // system_dynamics_handler.py:119-122 (x - mu)/(sd + 1e-7)
        if (f < S) {
            tmean[f] = normd ? m.mean_t[f] : 0.0f;
            tstd[f] = normd ? (m.std_t[f] + 1e-7f) : 1.0f;
            lbias[f] = (m.bpack[L - 1] + e * q.bstride[L - 1])[((size_t)(f >> 4) * 64 + ((f & 15) >> 2) * 16) * 4 + (f & 3)];
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
        for (int j = 0; j < MLP_PART_PF; ++j) en[j] = nbase[j] >= 0 ? nsig[j] * pa.pnoise[nbase[j] + t * S] : 0.0f;
        // ---- dense layers (kernels_mlp.hpp, SPEC 0) on member e's operands
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            mlp_layer_out_split_member<EXT>(m, q.wp4[l] + e * q.wstride[l], m.bpack[l] + e * q.bstride[l], l, in_off, out_off, wave, lane, nw);
            __syncthreads();
            in_off = out_off;
        }
        mlp_layer_k_split(m, q.wp4[L - 1] + e * q.wstride[L - 1], L - 1, in_off, lay.part, wave, lane, nw);
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
