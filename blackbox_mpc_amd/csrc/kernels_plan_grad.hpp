// Plan gradients (bbmpc_plan_gradient): G[b, t, u] = dR[b] / da_t[u] of the model return
//     R[b] = sum over t ascending of r(s_t, a_t, s_{t+1}) + w * V(s_Hq),      s_{t+1} = s_t + denorm(DynStack(norm(s_t, a_t)))
// through the learned dynamics (bbmpc_set_mlp), the learned reward (bbmpc_set_reward_mlp) and, when installed, the learned
// terminal value (bbmpc_set_terminal_value_mlp), by reverse accumulation.
//
// ONE kernel, k_plan_grad.  A workgroup owns 16 rows of the batch (the MFMA N dimension, as k_traj_mlp) for the forward
// sweep t = 0 .. Hq-1 AND the backward sweep t = Hq-1 .. 0: the adjoint tile, the normalisation constants and the row's
// return never leave the CU, and what the backward sweep needs from the forward one -- act'(z) of every unit of every
// layer, nothing else: no state and no activation value enters a derivative once act' is known -- goes through a region of
// the handle's HBM workspace that belongs to this workgroup alone.
//
// Every Dense layer of both sweeps is mlp_layer_out_split (kernels_mlp.hpp: v_mfma_f32_16x16x4_f32, fp32 in / fp32
// accumulate, operands streamed from an [OT][IT][lane][4] copy made by mlp_pack_layer).  The forward sweep calls it on
// descriptors whose activation code is ACT_NONE, so the pre-activation tile z lands in LDS; the wave that owns an output
// tile then replaces z by act(z) in place and stores act'(z) (activations_grad.hpp) as one float4 per lane.  The backward
// sweep calls it on the REVERSED network -- layer j is W^T of layer L-1-j, packed by the same routine, bias zero, no
// activation -- and the owning wave multiplies the adjoint tile by the act' it stored itself in the forward sweep.  Output
// tiles are dealt to waves by the same rule in both directions (tile ot belongs to wave ot % nw), so a lane reads back
// exactly the addresses it wrote: program order, no fence.  The last (narrow) layers run through the same routine; the
// K-split form with its nw x OT partial-sum block does not fit the LDS beside three networks at the limits.
//
// No atomics; nothing depends on the grid: two runs give equal bits and a batch split at a multiple of 16 equals the whole.
// Rows b >= B roll zeros and are neither read nor written.
#pragma once
#include "activations_grad.hpp"
#include "kernels_mlp.hpp"

namespace bbmpc {

struct PgNet {
    MlpDesc f;                               // forward: dims, tiles, bpack (every layer, the last one too); act[] = ACT_NONE
    MlpDesc r;                               // reversed: dims[j] = f.dims[L - j], bpack = zeros, act[] = ACT_NONE
    const float* wf[MLP_MAX_LAYERS];         // forward operands [OT][IT][64][4], features in index order
    const float* wr[MLP_MAX_LAYERS];         // wr[j]: layer L-1-j transposed, same layout
    int act[MLP_MAX_LAYERS];                 // the network's activation codes
    int hid;                                 // hidden 16-feature tiles, summed over layers 1 .. L-1
};

struct PlanGradArgs {
    PgNet dyn, rew, val;                     // dyn.f carries the model's statistics pointers (mean_s .. std_t)
    int has_val;
    float w;                                 // terminal_weight
    int nw, B, Hq, S, U;
    int r_norm, r_mask, r_D, r_off_a, r_off_n;       // the reward network's input: RewMlpDesc's fields
    const float* r_mean;                     // [D]
    const float* r_std;                      // [D]
    float r_mean_out, r_std_out;
    int v_norm;
    const float* v_mean;                     // [S]
    const float* v_std;                      // [S]
    float v_mean_out, v_std_out;
    int step_stride, tile_stride;            // workspace floats per (tile, step) and per tile
    const float* states;                     // [B, S]
    const float* seq;                        // [B, Hq, U]
    float* returns_out;                      // [B] or null
    float* grad_out;                         // [B, Hq, U]
    float* ws;                               // [tiles][tile_stride]
};

// Workspace of one tile, in floats: Hq steps of { dynamics hidden act' [dyn.hid][64][4] | dynamics output act' [16 * S] |
// reward hidden act' [rew.hid][64][4] | reward output act' [16] }, then { value hidden act' [val.hid][64][4] }.
__host__ __device__ inline int plan_grad_step_stride(int dyn_hid, int rew_hid, int S) { return (dyn_hid + rew_hid) * 256 + 16 * S + 16; }

// LDS carve in floats (pieces are multiples of 4 floats):
//   xd   [IT0 dyn][64][4]    the dynamics' normalised input tile; the backward sweep's seed tile of the dynamics
//   xr   [max(IT0 reward, IT0 value)][64][4]   the reward's / the value's input tile; their seed tile
//   actA / actB [ITmax][64][4]    ping-pong, ITmax over every layer width of the three networks, inputs included
//   st   [2][16][Sp]         raw state, double buffered
//   lam  [16][Sp]            the adjoint dR/ds_{t+1}
//   gs   [16][Sp]            dr_t/ds_t
//   ga   [16][U]             dr_t/da_t
//   acts [2][16][U]          raw actions of step t and t + 1
//   norm                     dynamics: mean, 1/(std+1e-7) [S+U], target mean, std+1e-7 [S] | reward: mean, std+1e-7 [D] | value: [S]
struct PgLds {
    int xd, xr, xr_n, actA, actB, st, lam, gs, ga, acts, norm, total;
};
__host__ __device__ inline PgLds plan_grad_lds_layout(const PgNet& d, const PgNet& r, const PgNet& v, int has_val, int S, int U, int D) {
    PgLds l;
    int itmax = 1;
    for (int i = 0; i <= d.f.n_layers; ++i) itmax = itmax > d.f.tiles[i] ? itmax : d.f.tiles[i];
    for (int i = 0; i <= r.f.n_layers; ++i) itmax = itmax > r.f.tiles[i] ? itmax : r.f.tiles[i];
    if (has_val)
        for (int i = 0; i <= v.f.n_layers; ++i) itmax = itmax > v.f.tiles[i] ? itmax : v.f.tiles[i];
    const int Sp = (S + 3) & ~3;
    int xr_t = r.f.tiles[0];
    if (has_val && v.f.tiles[0] > xr_t) xr_t = v.f.tiles[0];
    int o = 0;
    l.xd = o;   o += d.f.tiles[0] * 256;
    l.xr = o;   l.xr_n = xr_t * 256; o += l.xr_n;
    l.actA = o; o += itmax * 256;
    l.actB = o; o += itmax * 256;
    l.st = o;   o += 2 * MLP_TP * Sp;
    l.lam = o;  o += MLP_TP * Sp;
    l.gs = o;   o += MLP_TP * Sp;
    l.ga = o;   o += ((MLP_TP * U + 3) & ~3);
    l.acts = o; o += ((2 * MLP_TP * U + 3) & ~3);
    l.norm = o; o += (((S + U) * 2 + S * 2 + D * 2 + S * 2 + 63) & ~63);
    l.total = o;
    return l;
}

#ifdef BBMPC_TU_MLP

// The forward stack on the input tile at in_off.  Hidden layers leave act(z) in LDS and act'(z) in wsd (layer l = 1 .. L-1
// at the sum of the earlier hidden layers' tiles); the last layer leaves its PRE-activation tile, whose offset is returned
// (the frames apply the last activation where they read the outputs).  Ends with a barrier.
__device__ __forceinline__ int pg_forward(const PgNet& n, int in_off, const PgLds& lay, float* wsd, int wave, int lane, int nw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = n.f.n_layers;
    int off = 0;
    for (int l = 0; l < L; ++l) {
        const int out_off = (l & 1) ? lay.actB : lay.actA;
        mlp_layer_out_split<false>(n.f, n.wf[l], l, in_off, out_off, wave, lane, nw);
        if (l < L - 1) {
            const int OT = n.f.tiles[l + 1], a = n.act[l];
            for (int ot = wave; ot < OT; ot += nw) {               // the tiles this wave has just written
                f32x4* zp = reinterpret_cast<f32x4*>(smem + out_off + (ot * 64 + lane) * 4);
                const f32x4 z = *zp;
                f32x4 y, d;
                y.x = apply_act(z.x, a); y.y = apply_act(z.y, a); y.z = apply_act(z.z, a); y.w = apply_act(z.w, a);
                d.x = act_grad(z.x, y.x, a); d.y = act_grad(z.y, y.y, a); d.z = act_grad(z.z, y.z, a); d.w = act_grad(z.w, y.w, a);
                *zp = y;
                *reinterpret_cast<f32x4*>(wsd + off + (ot * 64 + lane) * 4) = d;
            }
            off += OT * 256;
        }
        __syncthreads();
        in_off = out_off;
    }
    return in_off;
}

// The backward stack: the tile at in_off holds dR/dz of the network's last layer (features past dims[L] zero); returns
// the offset of dR/dx, x the network's (normalised) input tile.  Ends with a barrier.
__device__ __forceinline__ int pg_backward(const PgNet& n, int in_off, const PgLds& lay, const float* wsd, int wave, int lane, int nw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int L = n.f.n_layers;
    for (int j = 0; j < L; ++j) {
        const int out_off = (j & 1) ? lay.actB : lay.actA;
        mlp_layer_out_split<false>(n.r, n.wr[j], j, in_off, out_off, wave, lane, nw);
        const int hl = L - 1 - j;                                  // the output is the adjoint of hidden layer hl's values (of the input: hl = 0)
        if (hl >= 1) {
            int off = 0;
            for (int l = 1; l < hl; ++l) off += n.f.tiles[l] * 256;
            const int OT = n.f.tiles[hl];
            for (int ot = wave; ot < OT; ot += nw) {
                f32x4* gp = reinterpret_cast<f32x4*>(smem + out_off + (ot * 64 + lane) * 4);
                const f32x4 d = *reinterpret_cast<const f32x4*>(wsd + off + (ot * 64 + lane) * 4);
                f32x4 g = *gp;
                g.x = g.x * d.x; g.y = g.y * d.y; g.z = g.z * d.z; g.w = g.w * d.w;
                *gp = g;
            }
        }
        __syncthreads();
        in_off = out_off;
    }
    return in_off;
}

// a one-output network's seed tile at `off`: feature 0 of row p <- seed (threads < 16 pass their row's), the rest zero
__device__ __forceinline__ void pg_seed_scalar(int off, float seed, int tid, int nthr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    for (int i = tid; i < 256; i += nthr) smem[off + i] = 0.0f;
    __syncthreads();
    if (tid < MLP_TP) smem[off + tile_addr(0, tid)] = seed;
    __syncthreads();
}

__global__ void k_plan_grad(PlanGradArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int n0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = q.S, U = q.U, D = q.r_D, Hq = q.Hq, B = q.B;
    const int Sp = (S + 3) & ~3;
    const MlpDesc& m = q.dyn.f;
    const int Ld = m.n_layers, Lr = q.rew.f.n_layers, Lv = q.val.f.n_layers;
    const PgLds lay = plan_grad_lds_layout(q.dyn, q.rew, q.val, q.has_val, S, U, D);
    float* xd = smem + lay.xd;
    float* xr = smem + lay.xr;
    float* st = smem + lay.st;
    float* lam = smem + lay.lam;
    float* gs = smem + lay.gs;
    float* ga = smem + lay.ga;
    float* acts = smem + lay.acts;
    float* nmean = smem + lay.norm;             // [S+U] input means (0 when not normalised)
    float* ninv = nmean + (S + U);              // [S+U] 1/(std + 1e-7)   (1 when not normalised)
    float* tmean = ninv + (S + U);              // [S] target mean
    float* tstd = tmean + S;                    // [S] target std + 1e-7
    float* rmean = tstd + S;                    // [D] the reward network's input mean
    float* rden = rmean + D;                    // [D] ... std + 1e-7
    float* vmean = rden + D;                    // [S] the value network's
    float* vden = vmean + S;                    // [S]
    const bool normd = m.normalized != 0;
    float* wst = q.ws + blockIdx.x * q.tile_stride;                 // this workgroup's region
    const int o_dl = q.dyn.hid * 256, o_rh = o_dl + 16 * S, o_rl = o_rh + q.rew.hid * 256;

    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? m.mean_s[f] : m.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? m.std_s[f] : m.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;              // k_traj_mlp's rule
        if (f < S) {
            tmean[f] = normd ? m.mean_t[f] : 0.0f;
            tstd[f] = normd ? (m.std_t[f] + 1e-7f) : 1.0f;
            vmean[f] = (q.has_val && q.v_norm) ? q.v_mean[f] : 0.0f;
            vden[f] = (q.has_val && q.v_norm) ? q.v_std[f] + 1e-7f : 1.0f;
        }
    }
    for (int k = tid; k < D; k += nthr) {
        rmean[k] = q.r_norm ? q.r_mean[k] : 0.0f;
        rden[k] = q.r_norm ? q.r_std[k] + 1e-7f : 1.0f;           // bbmpc_process_input's epsilon
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) xd[i] = 0.0f;
    for (int i = tid; i < lay.xr_n; i += nthr) xr[i] = 0.0f;
    for (int i = tid; i < MLP_TP * S; i += nthr) {
        const int pp = i / S, s = i - pp * S;
        st[pp * Sp + s] = (n0 + pp < B) ? q.states[(size_t)(n0 + pp) * S + s] : 0.0f;
    }
    for (int e = tid; e < MLP_TP * U; e += nthr) {                 // the actions of step 0 (rows past the batch roll zeros)
        const int pp = e / U, u = e - pp * U;
        acts[e] = (n0 + pp < B) ? q.seq[((size_t)(n0 + pp) * Hq) * U + u] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < MLP_TP * (S + U); i += nthr) {           // normalised layer-0 input for t = 0
        const int f = i >> 4, pp = i & 15;
        const float v = (f < S) ? st[pp * Sp + f] : acts[pp * U + (f - S)];
        xd[tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
    }
    __syncthreads();

    // ---------------------------------------------------------------- forward sweep
    float ret = 0.0f;                                               // threads < 16: the row's return
    for (int t = 0; t < Hq; ++t) {
        float* cur = st + (t & 1) * MLP_TP * Sp;
        float* nxt = st + ((t + 1) & 1) * MLP_TP * Sp;
        const float* act_t = acts + (t & 1) * MLP_TP * U;
        float* act_n = acts + ((t + 1) & 1) * MLP_TP * U;
        const bool more = t + 1 < Hq;
        float* wss = wst + t * q.step_stride;
        const int zd = pg_forward(q.dyn, lay.xd, lay, wss, wave, lane, nw);
        // ---- the model's epilogue (k_traj_mlp's): last activation, de-normalise, residual; the next step's input
        const int ad = q.dyn.act[Ld - 1];
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int f = i >> 4, pp = i & 15;
            const float z = smem[zd + tile_addr(f, pp)];
            const float y = apply_act(z, ad);
            wss[o_dl + i] = act_grad(z, y, ad);
            const float dev = normd ? tmean[f] + y * tstd[f] : y;
            const float ns = dev + cur[pp * Sp + f];
            nxt[pp * Sp + f] = ns;
            xd[tile_addr(f, pp)] = (ns - nmean[f]) * ninv[f];
        }
        for (int e = tid; e < MLP_TP * U; e += nthr) {
            const int pp = e / U, u = e - pp * U;
            const float v = (more && n0 + pp < B) ? q.seq[((size_t)(n0 + pp) * Hq + (t + 1)) * U + u] : 0.0f;
            act_n[e] = v;
            xd[tile_addr(S + u, pp)] = (v - nmean[S + u]) * ninv[S + u];
        }
        __syncthreads();
        // ---- the reward network on (s_t, a_t, s_{t+1}) (k_reward_mlp_rows' input rule)
        for (int i = tid; i < MLP_TP * D; i += nthr) {
            const int pp = i / D, k = i - pp * D;
            float v = 0.0f;
            if (n0 + pp < B) {
                if ((q.r_mask & 1) && k < S) v = cur[pp * Sp + k];
                else if ((q.r_mask & 2) && k < q.r_off_a + U) v = act_t[pp * U + (k - q.r_off_a)];
                else v = nxt[pp * Sp + (k - q.r_off_n)];
                v = (v - rmean[k]) / rden[k];
            }
            xr[tile_addr(k, pp)] = v;
        }
        __syncthreads();
        const int zr = pg_forward(q.rew, lay.xr, lay, wss + o_rh, wave, lane, nw);
        if (tid < MLP_TP) {
            const int ar = q.rew.act[Lr - 1];
            const float z = smem[zr + tile_addr(0, tid)];
            const float y = apply_act(z, ar);
            wss[o_rl + tid] = act_grad(z, y, ar);
            ret = ret + (q.r_norm ? y * q.r_std_out + q.r_mean_out : y);
        }
        __syncthreads();
    }

    // ---------------------------------------------------------------- the terminal value and lambda_Hq = w * grad V
    const float* s_last = st + (Hq & 1) * MLP_TP * Sp;
    if (q.has_val) {
        float* wsv = wst + Hq * q.step_stride;
        for (int i = tid; i < lay.xr_n; i += nthr) xr[i] = 0.0f;
        __syncthreads();
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int pp = i / S, k = i - pp * S;
            xr[tile_addr(k, pp)] = (n0 + pp < B) ? (s_last[pp * Sp + k] - vmean[k]) / vden[k] : 0.0f;
        }
        __syncthreads();
        const int zv = pg_forward(q.val, lay.xr, lay, wsv, wave, lane, nw);
        float seed = 0.0f;
        if (tid < MLP_TP) {
            const int av = q.val.act[Lv - 1];
            const float z = smem[zv + tile_addr(0, tid)];
            const float y = apply_act(z, av);
            const float dv = act_grad(z, y, av);
            ret = ret + q.w * (q.v_norm ? y * q.v_std_out + q.v_mean_out : y);
            seed = q.w * ((q.v_norm ? q.v_std_out : 1.0f) * dv);
        }
        __syncthreads();
        pg_seed_scalar(lay.xr, seed, tid, nthr);
        const int gv = pg_backward(q.val, lay.xr, lay, wsv, wave, lane, nw);
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int f = i >> 4, pp = i & 15;
            lam[pp * Sp + f] = smem[gv + tile_addr(f, pp)] / vden[f];
        }
    } else {
        for (int i = tid; i < MLP_TP * Sp; i += nthr) lam[i] = 0.0f;
    }
    if (q.returns_out && tid < MLP_TP && n0 + tid < B) q.returns_out[n0 + tid] = ret;
    __syncthreads();

    // ---------------------------------------------------------------- backward sweep
    const int OTd = m.tiles[Ld];
    for (int t = Hq - 1; t >= 0; --t) {
        const float* wss = wst + t * q.step_stride;
        // ---- the reward of step t: dr/ds_{t+1} joins lambda_{t+1}; dr/ds_t and dr/da_t wait in gs / ga
        const float rseed = tid < MLP_TP ? (q.r_norm ? q.r_std_out : 1.0f) * wss[o_rl + tid] : 0.0f;
        pg_seed_scalar(lay.xr, rseed, tid, nthr);
        const int gr = pg_backward(q.rew, lay.xr, lay, wss + o_rh, wave, lane, nw);
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int f = i >> 4, pp = i & 15;
            gs[pp * Sp + f] = (q.r_mask & 1) ? smem[gr + tile_addr(f, pp)] / rden[f] : 0.0f;
            if (q.r_mask & 4) lam[pp * Sp + f] = lam[pp * Sp + f] + smem[gr + tile_addr(q.r_off_n + f, pp)] / rden[q.r_off_n + f];
        }
        for (int e = tid; e < MLP_TP * U; e += nthr) {
            const int pp = e / U, u = e - pp * U;
            ga[e] = (q.r_mask & 2) ? smem[gr + tile_addr(q.r_off_a + u, pp)] / rden[q.r_off_a + u] : 0.0f;
        }
        __syncthreads();
        // ---- the model step: seed = lambda_{t+1} * d(s_{t+1}) / dz of the last layer
        for (int i = tid; i < OTd * 256; i += nthr) {
            const int f = i >> 4, pp = i & 15;
            xd[tile_addr(f, pp)] = f < S ? lam[pp * Sp + f] * tstd[f] * wss[o_dl + i] : 0.0f;
        }
        __syncthreads();
        const int gd = pg_backward(q.dyn, lay.xd, lay, wss, wave, lane, nw);
        for (int i = tid; i < MLP_TP * S; i += nthr) {
            const int f = i >> 4, pp = i & 15;
            lam[pp * Sp + f] = (gs[pp * Sp + f] + lam[pp * Sp + f]) + smem[gd + tile_addr(f, pp)] * ninv[f];
        }
        for (int e = tid; e < MLP_TP * U; e += nthr) {
            const int pp = e / U, u = e - pp * U;
            const float g = ga[e] + smem[gd + tile_addr(S + u, pp)] * ninv[S + u];
            if (n0 + pp < B) q.grad_out[((size_t)(n0 + pp) * Hq + t) * U + u] = g;
        }
        __syncthreads();
    }
}

#endif  // BBMPC_TU_MLP

}  // namespace bbmpc
