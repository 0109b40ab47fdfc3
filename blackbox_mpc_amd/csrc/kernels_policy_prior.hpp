// Learned policy prior (bbmpc_set_policy_prior_mlp): closed-loop rollouts of a policy network pi
// through the learned model, written straight into candidate columns of CEM's sample buffer,
//     a_t = clip(pi(s_t) + sigma_pi * xi[a, e, t, :], lo, hi)        s_{t+1} = the learned model's noise-free step (s_t, a_t)
//     pi(s) = denorm(Dense stack((s - mean_in) / (std_in + 1e-7)))   y * std_out + mean_out when normalised, y otherwise
// One kernel alternates the two Dense stacks for H steps on 16-row tiles:
//   k_policy_prior_rollout<EXT>   grid (ceil(K / 16), A): a workgroup owns 16 policy rollouts of one agent.  Per step the
//                       policy stack runs on the state tile (the generic rollout's layers, kernels_mlp.hpp SPEC 0:
//                       v_mfma_f32_16x16x4_f32, hidden layers output-tile split, the U-wide last layer K split), its
//                       epilogue de-normalises, adds the noise, clips and leaves the action in the model's input tile, in
//                       the sample buffer samples[(a * HU + t * U + u) * Nst + col0 + e] and (bbmpc_predict_policy_rollouts) in
//                       actions_out [K, A, H, U]; then the dynamics stack runs on (state, action) and its epilogue makes the
//                       next state tile, which goes to states_out [K, A, H, S] when asked.  The step's noise elements are
//                       fetched before the policy stack and held in registers.  Rows e >= K are neither read nor written.
//   k_policy_prior_rows<EXT>      pi on B independent rows (bbmpc_evaluate_policy_prior): no noise, no clip.
//   k_gen_policy_noise  the stream BBMPC_NOISE_POLICY, k_gen_process_noise's keying with 12 for 11, U for S, e for p.
// The dynamics prologue (normalisation constants, input staging) and epilogue (partial sums, bias, de-normalise, residual)
// restate k_traj_mlp of kernels_mlp_traj.hpp, which restates rollout_mlp_body<0> of kernels_mlp.hpp: a fix in one belongs
// in the others as well.  The K loops are those of mlp_layer_out_split / mlp_layer_k_split themselves, not typed-pointer
// restatements as in kernels_reward_mlp.hpp: the LDS tiles are offsets into the dynamic array and the operand pointers come
// in through the kernel-argument struct, which is what lets the compiler keep both address spaces (DESIGN.md section 8l
// records the ISA: no flat load, no scratch; check it again after any edit to this frame).  No atomics: the result does
// not depend on the grid, on the number of agents or on the run.  Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp.hpp"

namespace bbmpc {

constexpr uint32_t NOISE_POLICY = 12u;       // BBMPC_NOISE_POLICY
constexpr int POLICY_MAX_HIDDEN = 512;

struct PolicyPriorArgs {
    MlpDesc m;                               // the learned model (Engine::mlp)
    const float* wp4[MLP_MAX_LAYERS];        // its operands [OT][IT][64 lanes][4]
    // the policy: dims[0] = S, dims[L] = U, features in index order (no half tails); mean_s / std_s hold mean_in / std_in
    // [S], mean_t / std_t hold mean_out / std_out [U]
    MlpDesc pm;
    const float* pwp4[MLP_MAX_LAYERS];
    int nw;                                  // waves per workgroup (the wider of the two networks decides)
    int K, A, H, S, U;
    int Nst, col0;                           // candidate stride of `samples` and the first policy column
    float sigma;                             // sigma_pi
    const float* state;                      // [A][S]
    const float* noise;                      // [A][K][H][U] standard normals (never read when sigma == 0)
    const float* lo;                         // [U]
    const float* hi;                         // [U]
    float* samples;                          // [A][H*U][Nst] or null
    float* actions_out;                      // [K][A][H][U] or null
    float* states_out;                       // [K][A][H][S] or null
};

struct PolicyRowsArgs {
    MlpDesc pm;
    const float* pwp4[MLP_MAX_LAYERS];
    int nw, B, S, U;
    const float* states;                     // [B][S]
    float* actions;                          // [B][U]
};

// LDS carve in floats (pieces are multiples of 4 floats):
//   xs [IT0][64][4] the model's normalised input tile | pxs [PIT0][64][4] the policy's | actA / actB [ITmax][64][4] ping-pong
//   of both stacks | part [nw][OTmax][64][4] the K-split partial sums of either last layer | st [2][16][Sp] raw states |
//   norm: the model's constants as MlpTrajLds::norm, then the policy's (mean_in, std_in + 1e-7) [S], (mean_out, std_out,
//   last bias, lo, hi) [U].  (No raw action tile: the model reads the action, normalised, from xs; nothing else needs it.)
struct PolicyPriorLds {
    int xs, pxs, actA, actB, part, st, norm, pnorm, total;
};
__host__ __device__ inline PolicyPriorLds policy_prior_lds_layout(const MlpDesc& m, const MlpDesc& pm, int U, int S, int nw) {
    PolicyPriorLds l;
    int itmax = 1;
    for (int i = 1; i < m.n_layers; ++i) itmax = itmax > m.tiles[i] ? itmax : m.tiles[i];
    for (int i = 1; i < pm.n_layers; ++i) itmax = itmax > pm.tiles[i] ? itmax : pm.tiles[i];
    const int otmax = m.tiles[m.n_layers] > pm.tiles[pm.n_layers] ? m.tiles[m.n_layers] : pm.tiles[pm.n_layers];
    const int Sp = (S + 3) & ~3;
    int o = 0;
    l.xs = o;    o += m.tiles[0] * 256;
    l.pxs = o;   o += pm.tiles[0] * 256;
    l.actA = o;  o += itmax * 256;
    l.actB = o;  o += itmax * 256;
    l.part = o;  o += nw * otmax * 256;
    l.st = o;    o += 2 * MLP_TP * Sp;
    l.norm = o;  o += (((S + U) * 2 + S * 3 + 63) & ~63);
    l.pnorm = o; o += ((S * 2 + U * 5 + 63) & ~63);
    l.total = o;
    return l;
}
// the rows frame: pxs | actA | actB | part | pnorm
__host__ __device__ inline PolicyPriorLds policy_rows_lds_layout(const MlpDesc& pm, int U, int S, int nw) {
    PolicyPriorLds l;
    int itmax = 1;
    for (int i = 1; i < pm.n_layers; ++i) itmax = itmax > pm.tiles[i] ? itmax : pm.tiles[i];
    int o = 0;
    l.xs = o;
    l.pxs = o;   o += pm.tiles[0] * 256;
    l.actA = o;  o += itmax * 256;
    l.actB = o;  o += itmax * 256;
    l.part = o;  o += nw * pm.tiles[pm.n_layers] * 256;
    l.st = o; l.norm = o;
    l.pnorm = o; o += ((S * 2 + U * 5 + 63) & ~63);
    l.total = o;
    return l;
}

constexpr int POLICY_PF = 2;        // noise elements a thread holds in registers across a step's policy stack

#ifdef BBMPC_TU_MLP

// Element j = t * U + u of policy rollout e, global agent ga: counter (e, ga * Qk + (j >> 2), control step, (12 << 16) | iter),
// Qk = ceil(H * U / 4) in key.q_per_agent; Box-Muller on the word pairs.  One thread per Philox block writes its (up to)
// four elements.  out [A][K][HU]
static __global__ void k_gen_policy_noise(RngKey key, uint32_t iter, int A, int K, int HU, int agent_offset, float* out) {
    const int Qk = (HU + 3) >> 2;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= A * K * Qk) return;
    const int jq = idx % Qk, e = (idx / Qk) % K, a = idx / (Qk * K);
    const RngKey kk = rng_key_now(key);
    const U4 b = rng_block(kk, NOISE_POLICY, iter, (uint32_t)e, (uint32_t)(agent_offset + a), (uint32_t)(jq * 4));
    float z[4];
    words_to_normal2(b.x, b.y, z[0], z[1]);
    words_to_normal2(b.z, b.w, z[2], z[3]);
    float* row = out + ((size_t)a * K + e) * HU;
#pragma unroll
    for (int u = 0; u < 4; ++u)
        if (jq * 4 + u < HU) row[jq * 4 + u] = z[u];
}

// The policy's constants to LDS: (mean_in, std_in + 1e-7) per state feature, (mean_out, std_out, last bias) per action
// feature.  The caller fences.
__device__ __forceinline__ void policy_constants(const MlpDesc& pm, float* pnorm, int S, int U, int tid, int nthr) {
    const bool pn = pm.normalized != 0;
    const int Lp = pm.n_layers;
    float* pmean = pnorm;
    float* pden = pmean + S;
    float* omean = pden + S;
    float* ostd = omean + U;
    float* pbias = ostd + U;
    for (int f = tid; f < S; f += nthr) {
        pmean[f] = pn ? pm.mean_s[f] : 0.0f;
        pden[f] = pn ? pm.std_s[f] + 1e-7f : 1.0f;
    }
    for (int u = tid; u < U; u += nthr) {
        omean[u] = pn ? pm.mean_t[u] : 0.0f;
        ostd[u] = pn ? pm.std_t[u] : 1.0f;
        pbias[u] = pm.bpack[Lp - 1][((size_t)(u >> 4) * 64 + ((u & 15) >> 2) * 16) * 4 + (u & 3)];
    }
}

// The policy's Dense stack on the tile at in_off = lay.pxs; leaves the last layer's partial sums in lay.part, fenced.
template <bool EXT>
__device__ __forceinline__ void policy_stack(const MlpDesc& pm, const float* const* pwp4, const PolicyPriorLds& lay, int wave, int lane, int nw) {
    const int Lp = pm.n_layers;
    int in_off = lay.pxs;
    for (int l = 0; l < Lp - 1; ++l) {
        const int out_off = (l & 1) ? lay.actB : lay.actA;
        mlp_layer_out_split<EXT>(pm, pwp4[l], l, in_off, out_off, wave, lane, nw);
        __syncthreads();
        in_off = out_off;
    }
    mlp_layer_k_split(pm, pwp4[Lp - 1], Lp - 1, in_off, lay.part, wave, lane, nw);
    __syncthreads();
}

// pi's output u of row pp from the partial sums: bias first, partials in wave order, last activation, de-normalise
template <bool EXT>
__device__ __forceinline__ float policy_output(const MlpDesc& pm, const float* part, const float* pnorm, int S, int U, int nw, int u, int pp) {
    const int Lp = pm.n_layers, OTp = pm.tiles[Lp];
    const int nwp = min(nw, pm.tiles[Lp - 1]);            // waves that actually produced partials
    const float* omean = pnorm + 2 * S;
    const float* ostd = omean + U;
    const float* pbias = ostd + U;
    const int ot = u >> 4, ln = ((u & 15) >> 2) * 16 + pp, rg = u & 3;
    const float* pp0 = part + (((size_t)ot) * 64 + ln) * 4 + rg;
    float acc = pbias[u];
    for (int w = 0; w < nwp; ++w) acc = acc + pp0[(size_t)w * OTp * 256];
    acc = apply_act_rt<EXT>(acc, pm.act[Lp - 1]);
    return pm.normalized ? acc * ostd[u] + omean[u] : acc;
}

template <bool EXT>
__global__ void k_policy_prior_rollout(PolicyPriorArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& m = q.m;
    const MlpDesc& pm = q.pm;
    const int n0 = blockIdx.x * MLP_TP, a = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = q.S, U = q.U, H = q.H, K = q.K, L = m.n_layers;
    const int Sp = (S + 3) & ~3;
    const PolicyPriorLds lay = policy_prior_lds_layout(m, pm, U, S, nw);
    float* xs = smem + lay.xs;
    float* pxs = smem + lay.pxs;
    float* part = smem + lay.part;
    float* st = smem + lay.st;
    const bool normd = m.normalized != 0;
    float* nmean = smem + lay.norm;             // [S+U] input means (0 when not normalised)
    float* ninv = nmean + (S + U);              // [S+U] 1/(std + 1e-7)   (1 when not normalised)
    float* tmean = ninv + (S + U);              // [S] target mean
    float* tstd = tmean + S;                    // [S] target std + 1e-7
    float* lbias = tstd + S;                    // [S] bias of the model's last layer
    float* pnorm = smem + lay.pnorm;
    const float* pmean = pnorm;                 // [S] the policy's input mean
    const float* pden = pnorm + S;              // [S] its std + 1e-7
    float* blo = pnorm + 2 * S + 3 * U;         // [U] action bounds
    float* bhi = blo + U;

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
    policy_constants(pm, pnorm, S, U, tid, nthr);
    for (int u = tid; u < U; u += nthr) {
        blo[u] = q.lo[u];
        bhi[u] = q.hi[u];
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) xs[i] = 0.0f;
    for (int i = tid; i < pm.tiles[0] * 256; i += nthr) pxs[i] = 0.0f;
    for (int i = tid; i < MLP_TP * S; i += nthr) {
        const int pp = i / S, s = i % S;
        st[pp * Sp + s] = (n0 + pp < K) ? q.state[(size_t)a * S + s] : 0.0f;       // (rows past K roll zeros)
    }
    __syncthreads();
    for (int i = tid; i < MLP_TP * S; i += nthr) {                // both stacks' normalised state inputs for t = 0
        const int f = i / MLP_TP, pp = i % MLP_TP;
        const float v = st[pp * Sp + f];
        xs[tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
        pxs[tile_addr(f, pp)] = (v - pmean[f]) / pden[f];
    }
    __syncthreads();

    const int OTl = m.tiles[L];
    const int HU = H * U;
    const bool noisy = q.sigma != 0.0f;
    const float* nz = q.noise + ((size_t)a * K) * HU;              // this agent's [K][H][U]
    for (int t = 0; t < H; ++t) {
        float* cur = st + (t & 1) * MLP_TP * Sp;
        float* nxt = st + ((t + 1) & 1) * MLP_TP * Sp;
        // ---- the step's noise elements i = tid, tid + nthr of the tile [U][16]: in flight across the policy stack
        float pf[POLICY_PF];
#pragma unroll
        for (int j = 0; j < POLICY_PF; ++j) {
            const int i = tid + j * nthr;
            const int u = i >> 4, pp = i & 15;
            pf[j] = (noisy && i < MLP_TP * U && n0 + pp < K) ? nz[((size_t)(n0 + pp) * H + t) * U + u] : 0.0f;
        }
        // ---- the policy's Dense stack on the state tile
        policy_stack<EXT>(pm, q.pwp4, lay, wave, lane, nw);
        // ---- its epilogue: de-normalise, add the noise, clip; the action to the model's input tile and to the outputs
        for (int i = tid, j = 0; i < MLP_TP * U; i += nthr, ++j) {
            const int u = i >> 4, pp = i & 15;
            const int row = n0 + pp;
            float xi = 0.0f;
            if (j < POLICY_PF) xi = j == 0 ? pf[0] : pf[1];
            else if (noisy && row < K) xi = nz[((size_t)row * H + t) * U + u];     // wide actions on few waves: fetched here
            float v = policy_output<EXT>(pm, part, pnorm, S, U, nw, u, pp);
            v = v + q.sigma * xi;
            v = clipf(v, blo[u], bhi[u]);
            xs[tile_addr(S + u, pp)] = (v - nmean[S + u]) * ninv[S + u];
            if (row < K) {
                if (q.samples) q.samples[((size_t)a * HU + t * U + u) * q.Nst + q.col0 + row] = v;
                if (q.actions_out) q.actions_out[(((size_t)row * q.A + a) * H + t) * U + u] = v;
            }
        }
        __syncthreads();
        // ---- the model's dense layers (kernels_mlp.hpp, SPEC 0)
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            mlp_layer_out_split<EXT>(m, q.wp4[l], l, in_off, out_off, wave, lane, nw);
            __syncthreads();
            in_off = out_off;
        }
        mlp_layer_k_split(m, q.wp4[L - 1], L - 1, in_off, lay.part, wave, lane, nw);
        __syncthreads();
        // ---- epilogue: reduce partials, bias, last activation, de-normalise, residual; stage step t + 1's inputs
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
            pxs[tile_addr(f, pp)] = (ns - pmean[f]) / pden[f];
        }
        __syncthreads();
        // ---- the step's state tile overlaps the next step's policy stack: row by row (S contiguous floats each).  `nxt` is
        // next written behind step t + 1's model stack.
        if (q.states_out) {
            for (int i = tid; i < MLP_TP * S; i += nthr) {
                const int pp = i / S, s = i - pp * S;
                if (n0 + pp < K) q.states_out[(((size_t)(n0 + pp) * q.A + a) * H + t) * S + s] = nxt[pp * Sp + s];
            }
        }
    }
}

template <bool EXT>
__global__ void k_policy_prior_rows(PolicyRowsArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& pm = q.pm;
    const int r0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = q.S, U = q.U;
    const PolicyPriorLds lay = policy_rows_lds_layout(pm, U, S, nw);
    float* pxs = smem + lay.pxs;
    float* pnorm = smem + lay.pnorm;
    const float* pmean = pnorm;
    const float* pden = pnorm + S;
    policy_constants(pm, pnorm, S, U, tid, nthr);
    for (int i = tid; i < pm.tiles[0] * 256; i += nthr) pxs[i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < MLP_TP * S; i += nthr) {
        const int pp = i / S, s = i - pp * S;
        if (r0 + pp < q.B) pxs[tile_addr(s, pp)] = (q.states[(size_t)(r0 + pp) * S + s] - pmean[s]) / pden[s];
    }
    __syncthreads();
    policy_stack<EXT>(pm, q.pwp4, lay, wave, lane, nw);
    for (int i = tid; i < MLP_TP * U; i += nthr) {
        const int pp = i / U, u = i - pp * U;
        if (r0 + pp < q.B) q.actions[(size_t)(r0 + pp) * U + u] = policy_output<EXT>(pm, smem + lay.part, pnorm, S, U, nw, u, pp);
    }
}

#endif  // BBMPC_TU_MLP

}  // namespace bbmpc
