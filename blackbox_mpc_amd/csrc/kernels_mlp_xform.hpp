// Learned-model rollout with a user-supplied inverse target transform inlined (hiprtc).
//
// The reference's SystemDynamicsHandler.process_output (dynamics_handlers/system_dynamics_handler.py:128-161) de-normalises
// the model output and hands it to inverse_transform_targets_func(states, dev) -- by default `dev + states`
// (utils/transforms.py:34).  A custom transform is HIP source defining
//     __device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S);
// and this kernel is compiled at run time with it (rtc.hpp program_source), so the Dense stack stays on the matrix
// cores and the transform costs one inlined call per particle and step.
//
// Mapping: the generic kernel's (kernels_mlp.hpp:1-20).  One workgroup owns a 16-particle tile of one agent for the whole
// H-step recurrence; layers run transposed on v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate) with the operands set_mlp
// already uploads ([OT][IT][64 lanes][4], MlpDesc.wpack's copy d_wpack4); activation tiles stay in LDS and are addressed
// as offsets into the dynamic LDS array.  Per step the epilogue runs
//   1. reduce the K-split partials, bias, last activation, de-normalise  -> dev row per particle (LDS)
//   2. barrier
//   3. one lane per particle: bbmpc_user_inverse_transform_targets(cur, dev, next, S)
//   4. barrier
//   5. trajectory record (optional), stage step t+1's normalised input, reward of step t (built-in or user, inlined)
// Candidates come from the caller's sequences (SRC_REF) or from the sample buffer the engine filled (SRC_BUF); clip and
// penalty as bbmpc_user_rollout (rtc.hpp) applies them.
//
// Only leaf headers that hiprtc receives (activations.hpp, models.hpp, fastmath.hpp) are included: the host side includes this file for
// XformArgs and the LDS layout; the kernel itself is compiled only where BBMPC_XFORM_KERNEL is defined (hiprtc).
#pragma once
#include <hip/hip_runtime.h>

#include "activations.hpp"   // apply_act: the generic kernel's activations, the same text
#include "models.hpp"

namespace bbmpc {

constexpr int XF_TP = 16;          // particles per workgroup tile
constexpr int XF_MAX_LAYERS = 8;

struct XformArgs {
    int n_pop, A, H, Nst;
    int from_ref;                      // 1: seq is the caller's [n_pop, A, H, U]; 0: cand is the internal layout [A][H*U][Nst]
    int pen;                           // clip + penalty
    int fix_q1;
    int nw;                            // waves per workgroup
    int n_layers;
    int normalized;
    int tiles[XF_MAX_LAYERS + 1];      // ceil(dims / 16)
    int act[XF_MAX_LAYERS];
    const float* wp4[XF_MAX_LAYERS];   // [OT][IT][64][4]
    const float* bpack[XF_MAX_LAYERS]; // [OT][64][4]
    const float* mean_s;               // [S]   (normalised models only)
    const float* std_s;
    const float* mean_a;               // [U]
    const float* std_a;
    const float* mean_t;               // [S]
    const float* std_t;
    const float* state;                // [A,S]
    const float* seq;
    const float* cand;
    float* samples;                    // the feasible candidates go back here (pen, SRC_BUF), or null
    const float* lo;
    const float* hi;
    float* rewards;                    // [A][Nst]
    float* penalty_out;                // optional [A][Nst]
    float* traj;                       // optional [H][A][Nst][S]: the state after every step
};

// LDS carve in floats (every piece a multiple of 4 floats):
//   xs [IT0][64][4] | actA, actB [ITmax][64][4] | part [nw][OTlast][64][4] | st [2][16][Sp] | dev [16][Sp] |
//   acts [H][16][U] | pens [16] | norm: mean, 1/(std+1e-7) of the inputs [S+U] each, mean_t, std_t+1e-7, last bias [S] each
struct XformLds {
    int xs, actA, actB, part, st, dev, acts, pens, norm, total;
};
__host__ __device__ inline XformLds xform_lds_layout(const int* tiles, int n_layers, int H, int S, int U, int nw) {
    XformLds l;
    int itmax = 1;
    for (int i = 1; i < n_layers; ++i) itmax = itmax > tiles[i] ? itmax : tiles[i];
    const int Sp = (S + 3) & ~3;
    int o = 0;
    l.xs = o;   o += tiles[0] * 256;
    l.actA = o; o += itmax * 256;
    l.actB = o; o += itmax * 256;
    l.part = o; o += nw * tiles[n_layers] * 256;
    l.st = o;   o += 2 * XF_TP * Sp;
    l.dev = o;  o += XF_TP * Sp;
    l.acts = o; o += (H * XF_TP * U + 3) & ~3;
    l.pens = o; o += XF_TP;
    l.norm = o; o += ((S + U) * 2 + S * 3 + 3) & ~3;
    l.total = o;
    return l;
}

#ifdef BBMPC_XFORM_KERNEL
typedef float xf_f32x4 __attribute__((ext_vector_type(4)));

// BBMPC_ACT_EXT=1: the network has an activation after sigmoid (activations.hpp); the program is compiled for the network
#ifndef BBMPC_ACT_EXT
#define BBMPC_ACT_EXT 1
#endif
constexpr bool XF_EXT = BBMPC_ACT_EXT != 0;

// the dynamic LDS array, declared once at namespace scope (the kernel has C linkage, the helpers do not)
extern __shared__ __attribute__((aligned(16))) float xf_smem[];

// feature f of particle p inside a tile array [T][64][4]
__device__ __forceinline__ int xf_tile_addr(int f, int p) {
    return (((f >> 4) * 64) + (((f & 15) >> 2) * 16 + p)) * 4 + (f & 3);
}

// hidden layer, output tiles dealt round-robin to the waves; in / out are LDS offsets
__device__ __forceinline__ void xf_layer_out_split(const XformArgs& q, int l, int in_off, int out_off, int wave, int lane) {
    float* const smem = xf_smem;
    const float* in = smem + in_off;
    float* out = smem + out_off;
    const int IT = q.tiles[l], OT = q.tiles[l + 1], a = q.act[l];
    const xf_f32x4* __restrict__ W = reinterpret_cast<const xf_f32x4*>(q.wp4[l]);
    for (int ot = wave; ot < OT; ot += q.nw) {
        xf_f32x4 acc = *reinterpret_cast<const xf_f32x4*>(q.bpack[l] + ((size_t)ot * 64 + lane) * 4);   // bias enters as C
        const xf_f32x4* w0 = W + (size_t)ot * IT * 64 + lane;
#pragma unroll 4
        for (int it = 0; it < IT; ++it) {
            const xf_f32x4 b = *reinterpret_cast<const xf_f32x4*>(in + ((size_t)it * 64 + lane) * 4);
            const xf_f32x4 w = w0[(size_t)it * 64];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, b.w, acc, 0, 0, 0);
        }
        acc = apply_act4<XF_EXT>(acc, a);
        *reinterpret_cast<xf_f32x4*>(out + ((size_t)ot * 64 + lane) * 4) = acc;
    }
}

// last layer, K split: the wave multiplies the input tiles it owns into every output tile; partial sums to part[wave]
__device__ __forceinline__ void xf_layer_k_split(const XformArgs& q, int l, int in_off, int part_off, int wave, int lane) {
    float* const smem = xf_smem;
    const float* in = smem + in_off;
    float* part = smem + part_off;
    const int IT = q.tiles[l], OT = q.tiles[l + 1];
    const xf_f32x4* __restrict__ W = reinterpret_cast<const xf_f32x4*>(q.wp4[l]);
    for (int ot = 0; ot < OT; ++ot) {
        xf_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int it = wave; it < IT; it += q.nw) {
            const xf_f32x4 b = *reinterpret_cast<const xf_f32x4*>(in + ((size_t)it * 64 + lane) * 4);
            const xf_f32x4 w = W[((size_t)ot * IT + it) * 64 + lane];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w.w, b.w, acc, 0, 0, 0);
        }
        *reinterpret_cast<xf_f32x4*>(part + (((size_t)wave * OT + ot) * 64 + lane) * 4) = acc;
    }
}

// grid (ceil(n_pop / 16), A), block nw * 64, dynamic LDS xform_lds_layout(...).total floats.  A parameterised user reward
// (BBMPC_REW_NPARAMS, rtc.hpp) takes rew_params [A][P] as a second argument and reads the row of agent blockIdx.y.
#ifdef BBMPC_REW_NPARAMS
extern "C" __global__ void bbmpc_mlp_xform_rollout(XformArgs q, const float* __restrict__ rew_params) {
#else
extern "C" __global__ void bbmpc_mlp_xform_rollout(XformArgs q) {
#endif
    constexpr int S = BBMPC_S, U = BBMPC_U, TP = XF_TP, Sp = (S + 3) & ~3;
    float* const smem = xf_smem;
    const int a = blockIdx.y, n0 = blockIdx.x * TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = q.nw * 64;
    const int L = q.n_layers, H = q.H, HU = H * U;
    const XformLds lay = xform_lds_layout(q.tiles, L, H, S, U, q.nw);
    float* xs = smem + lay.xs;
    float* part = smem + lay.part;
    float* st = smem + lay.st;
    float* devb = smem + lay.dev;
    float* acts = smem + lay.acts;
    float* pens = smem + lay.pens;
    float* nmean = smem + lay.norm;             // [S+U] input means (0 when not normalised)
    float* ninv = nmean + (S + U);              // [S+U] 1/(std + 1e-7)   (1 when not normalised)
    float* tmean = ninv + (S + U);              // [S] target mean
    float* tstd = tmean + S;                    // [S] target std + 1e-7
    float* lbias = tstd + S;                    // [S] bias of the last layer
    const bool normd = q.normalized != 0;

    // ---- prologue: statistics, start state, the tile's action block [H][16][U]
    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? q.mean_s[f] : q.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? q.std_s[f] : q.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;                      // system_dynamics_handler.py:119-122
        if (f < S) {
            tmean[f] = normd ? q.mean_t[f] : 0.0f;
            tstd[f] = normd ? (q.std_t[f] + 1e-7f) : 1.0f;
            lbias[f] = q.bpack[L - 1][((size_t)(f >> 4) * 64 + ((f & 15) >> 2) * 16) * 4 + (f & 3)];
        }
    }
    for (int i = tid; i < q.tiles[0] * 256; i += nthr) xs[i] = 0.0f;
    for (int i = tid; i < TP * S; i += nthr) st[(i / S) * Sp + (i % S)] = q.state[a * S + (i % S)];
    for (int e = tid; e < HU * TP; e += nthr) {             // particle fastest: coalesced reads of the internal layout
        const int pp = e % TP, j = e / TP, t = j / U, u = j - t * U, n = n0 + pp;
        float x = 0.0f;
        if (n < q.n_pop) x = q.from_ref ? q.seq[((size_t)n * q.A + a) * HU + j] : q.cand[((size_t)a * HU + j) * q.Nst + n];
        acts[(t * TP + pp) * U + u] = x;
    }
    __syncthreads();
    if (tid < TP) {
        // clip + squared bound violation in j = t*U + u order, as bbmpc_user_rollout / k_rows_prepare sum it
        float pen = 0.0f;
        const int n = n0 + tid;
        if (q.pen && n < q.n_pop) {
            for (int j = 0; j < HU; ++j) {
                const int t = j / U, u = j - t * U;
                float* slot = acts + (t * TP + tid) * U + u;
                const float x = *slot;
                const float xf = clipf(x, q.lo[u], q.hi[u]);
                const float d = x - xf;
                pen = pen + d * d;
                *slot = xf;
                if (q.samples) q.samples[((size_t)a * HU + j) * q.Nst + n] = xf;
            }
        }
        pens[tid] = pen;
    }
    __syncthreads();
    for (int i = tid; i < TP * (S + U); i += nthr) {           // normalised layer-0 input of step 0
        const int f = i / TP, pp = i % TP;
        const float v = f < S ? st[pp * Sp + f] : acts[pp * U + (f - S)];
        xs[xf_tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
    }
    __syncthreads();

    float total = 0.0f;                                       // lanes 0..15 of wave 0: particle `tid`
    const int OTl = q.tiles[L];
    const int nwp = q.nw < q.tiles[L - 1] ? q.nw : q.tiles[L - 1];      // waves that produce partials
    for (int t = 0; t < H; ++t) {
        float* cur = st + (t & 1) * TP * Sp;
        float* nxt = st + ((t + 1) & 1) * TP * Sp;
        // ---- dense layers
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            xf_layer_out_split(q, l, in_off, out_off, wave, lane);
            __syncthreads();
            in_off = out_off;
        }
        xf_layer_k_split(q, L - 1, in_off, lay.part, wave, lane);
        __syncthreads();
        // ---- 1. reduce, bias, last activation, de-normalise -> dev
        for (int i = tid; i < TP * S; i += nthr) {
            const int f = i / TP, pp = i % TP;
            const int ot = f >> 4, ln = ((f & 15) >> 2) * 16 + pp, rg = f & 3;
            const float* p0 = part + ((size_t)ot * 64 + ln) * 4 + rg;
            float acc = lbias[f];
            for (int w = 0; w < nwp; ++w) acc = acc + p0[(size_t)w * OTl * 256];
            acc = apply_act_rt<XF_EXT>(acc, q.act[L - 1]);
            devb[pp * Sp + f] = normd ? tmean[f] + acc * tstd[f] : acc;       // system_dynamics_handler.py:152-155
        }
        __syncthreads();
        // ---- 3. the user's inverse transform, one lane per particle
        if (tid < TP) bbmpc_user_inverse_transform_targets(cur + tid * Sp, devb + tid * Sp, nxt + tid * Sp, S);
        __syncthreads();
        // ---- 5. record, stage step t+1's input, reward of step t
        for (int i = tid; i < TP * (S + U); i += nthr) {
            const int f = i / TP, pp = i % TP;
            float v;
            if (f < S) {
                v = nxt[pp * Sp + f];
                if (q.traj && n0 + pp < q.n_pop) q.traj[((((size_t)t * q.A + a) * q.Nst) + n0 + pp) * S + f] = v;
            } else {
                const int tn = (t + 1 < H) ? t + 1 : t;
                v = acts[(tn * TP + pp) * U + (f - S)];
            }
            xs[xf_tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
        }
        __syncthreads();
        if (tid < TP) {
            const float* c = cur + tid * Sp;
            const float* ac = acts + (t * TP + tid) * U;
            const float* nx = nxt + tid * Sp;
#if BBMPC_REW_KIND == 3
            total = total + BBMPC_CALL_REWARD(c, ac, nx, rew_params, a, t);    // (current_state, actions, next_state); rtc.hpp k_user_calls
#else
            total = total + reward_generic(BBMPC_REW_KIND, q.fix_q1 != 0, c, ac, nx, S, U);
#endif
        }
    }
    if (tid < TP) {
        const int n = n0 + tid;
        if (n < q.n_pop) {
            if (total != total) total = -1.0e6f;                               // deterministic.py:75-77
            if (q.pen) {
                const float nr = sqrtf(pens[tid]);                             // tf.norm(...)**2  pi2.py:72-75
                const float pv = nr * nr;
                total = total - pv;
                if (q.penalty_out) q.penalty_out[(size_t)a * q.Nst + n] = pv;
            }
            q.rewards[(size_t)a * q.Nst + n] = total;
        }
    }
}
#endif  // BBMPC_XFORM_KERNEL

}  // namespace bbmpc
