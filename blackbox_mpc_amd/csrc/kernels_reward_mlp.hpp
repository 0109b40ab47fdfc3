// Learned reward models (BBMPC_REW_MLP, bbmpc_set_reward_mlp): a second Dense stack that maps
// (s_t, a_t, s_{t+1}) -- the blocks `input_mask` selects, concatenated in that order -- to ONE reward, run on the matrix
// cores over states the learned-model rollouts have already produced.
//
// Body (rew_mlp_stack): the generic rollout's layer (kernels_mlp.hpp, SPEC 0) on 16-row tiles -- v_mfma_f32_16x16x4_f32,
// fp32 in / fp32 accumulate, operands streamed from the packed [OT][IT][lane][4] copy that mlp_pack_layer makes, output
// tiles dealt round-robin to the waves, run-time activation codes through activations.hpp.  The weight / bias operands and
// the LDS tiles are read through address-space-typed pointers, so the K loop holds global_load_dwordx4 and ds_read_b128
// and no flat load (what a flat load in that loop costs: mlp_layer_out_split).  The last layer has one output: a
// reduction over the last hidden tile in a fixed order (16 rows x 4 * nw strided partial sums, then one lane per row adds
// the partials in index order), not an MFMA tile.  A 1-layer network is that reduction over the input tile alone.
//
// Two frames around it:
//   k_reward_mlp_traj   rows (n, t) of the rollout's trajectory buffer u_traj [H][A][Nst][S]: a workgroup owns 16
//                       candidates of one agent and a chunk of planning steps (grid = tiles x agents x t-chunks: steps are
//                       independent, so a small population still fills the GPU) and leaves every step's reward in
//                       step_out [H][A][Nst]; k_reward_mlp_finish then adds a candidate's H rewards in t order to what the
//                       rollout left in `rewards` (-penalty), NaN -> -1e6 per trajectory.  No atomics: the sum does not
//                       depend on the chunking, on the number of agents or on the run.
//   k_reward_mlp_rows   B independent rows with their own cur / act / nxt pointers and strides, one reward per row, no sum,
//                       no NaN rule (evaluate_next_reward, the control step's record, predict_trajectories).
// ... and a third for a learned terminal value (bbmpc_set_terminal_value_mlp), a network over the
// state alone (mask = s_t, D = S):
//   k_value_mlp_terminal  the 16 candidates' LAST recorded states (plane H - 1 of u_traj) through the stack, then lanes
//                       0..15 finish in place: rewards[a][n] += w * V(s_H), NaN -> -1e6.  One launch behind whatever scored
//                       the steps, no atomics.  k_reward_mlp_rows with the value network's descriptor serves
//                       bbmpc_evaluate_terminal_value.
#pragma once
#include "kernels_mlp.hpp"

namespace bbmpc {

constexpr int REW_MLP_MAX_IN = 192;          // D: dim_S <= 64 and dim_S + dim_U <= 128 (bbmpc_set_mlp), all three blocks
constexpr int REW_MLP_MAX_HIDDEN = 512;

struct RewMlpDesc {
    int n_layers;
    int dims[MLP_MAX_LAYERS + 1];            // dims[0] = D ... dims[L] = 1
    int tiles[MLP_MAX_LAYERS + 1];           // ceil(dims / 16)
    int act[MLP_MAX_LAYERS];
    const float* wp4[MLP_MAX_LAYERS];        // layers l < L - 1: [OT][IT][64 lanes][4] (mlp_pack_layer's w4)
    const float* bpack[MLP_MAX_LAYERS];      // layers l < L - 1: [OT][64][4]
    const float* wlast;                      // [dims[L - 1]]: the last Dense kernel's one column
    float blast;                             // its bias
    int mask, S, U, D;                       // input_mask (bit 0 s_t, bit 1 a_t, bit 2 s_{t+1}) and the blocks' widths
    int off_a, off_n;                        // first input column of the action block / of the next-state block
    int normalized;
    const float* mean_in;                    // [D]
    const float* std_in;                     // [D]
    float mean_r, std_r;
    int nw;                                  // waves per workgroup
};

// LDS carve in floats: xs [IT0][64][4] the (normalised) input tile | actA / actB [ITmax][64][4] ping-pong | red [nw * 64]
// the last layer's partial sums | norm [2][D] input mean and std + 1e-7
struct RewMlpLds {
    int xs, actA, actB, red, norm, total;
};
__host__ __device__ inline RewMlpLds rew_mlp_lds_layout(const RewMlpDesc& m) {
    RewMlpLds l;
    int itmax = 1;
    for (int i = 1; i < m.n_layers; ++i) itmax = itmax > m.tiles[i] ? itmax : m.tiles[i];
    int o = 0;
    l.xs = o;   o += m.tiles[0] * 256;
    l.actA = o; o += itmax * 256;
    l.actB = o; o += itmax * 256;
    l.red = o;  o += m.nw * 64;
    l.norm = o; o += ((2 * m.D + 63) & ~63);
    l.total = o;
    return l;
}

struct RewMlpTrajArgs {
    RewMlpDesc m;
    int n_pop, A, H, Nst, HU, from_ref;
    int tchunk;                              // planning steps per workgroup (grid.z = ceil(H / tchunk))
    const float* state;                      // [A][S]
    const float* traj;                       // [H][A][Nst][S] the state after every step
    const float* seq;                        // SRC_REF: [n_pop][A][HU]
    const float* cand;                       // else: [A][HU][Nst] (the feasible candidates where the rollout clipped them)
    float* step_out;                         // [H][A][Nst]
};

struct RewMlpRowsArgs {
    RewMlpDesc m;
    int B;
    // row r reads cur + (r - cur_shift) * cur_stride -- or, when `first` is set and r % period == 0, first + (r / period) * S
    // (predict_trajectories: the row's own start state at t = 0, states_out[b, t - 1] afterwards)
    int period, cur_shift;
    const float* first;
    const float* cur;
    const float* act;
    const float* nxt;
    long cur_stride, act_stride, nxt_stride;
    float* out;                              // [B]
};

struct ValMlpTermArgs {
    RewMlpDesc m;                            // mask = 1 (s_t), D = S
    int n_pop, A, Nst;
    float weight;                            // terminal_weight
    const float* last;                       // [A][Nst][S]: the trajectory buffer's last plane, u_traj + (H - 1) * A * Nst * S
    float* rewards;                          // [A][Nst]: the step sum (NaN -> -1e6) - penalty, finished in place
};

#ifdef BBMPC_TU_MLP

typedef __attribute__((address_space(3))) float rew_lds_f;
typedef const __attribute__((address_space(3))) f32x4 rew_lds_cf4;
typedef __attribute__((address_space(3))) f32x4 rew_lds_f4;
typedef const __attribute__((address_space(1))) f32x4 rew_glb_cf4;
typedef const __attribute__((address_space(1))) float rew_glb_cf;

// One hidden Dense layer, output-tile split: mlp_layer_out_split's schedule (two output tiles per pass on one LDS read of
// the input tile, a ring of MLP_GEN_PF operand tiles in registers) with typed pointers.
__device__ __forceinline__ void rew_mlp_layer(const RewMlpDesc& m, int l, int in_off, int out_off, int wave, int lane, int nw) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    rew_lds_f* lds = (rew_lds_f*)smem;
    rew_lds_cf4* in = (rew_lds_cf4*)(lds + in_off);
    rew_lds_f4* out = (rew_lds_f4*)(lds + out_off);
    const int IT = m.tiles[l], OT = m.tiles[l + 1];
    rew_glb_cf4* W = (rew_glb_cf4*)m.wp4[l];
    rew_glb_cf4* bp = (rew_glb_cf4*)m.bpack[l];
    const int a = m.act[l];
    for (int ot0 = wave; ot0 < OT; ot0 += 2 * nw) {
        const int ot1 = ot0 + nw;
        if (ot1 < OT) {
            f32x4 acc0 = bp[(size_t)ot0 * 64 + lane];      // bias enters as C
            f32x4 acc1 = bp[(size_t)ot1 * 64 + lane];
            rew_glb_cf4* w0 = W + (size_t)ot0 * IT * 64 + lane;
            rew_glb_cf4* w1 = W + (size_t)ot1 * IT * 64 + lane;
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
                        const f32x4 b = in[k * 64 + lane];
                        const f32x4 a0 = r0[j], a1 = r1[j];
                        const int kn = k + MLP_GEN_PF < IT ? k + MLP_GEN_PF : IT - 1;      // (the last refills re-read the last tile)
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
            out[ot0 * 64 + lane] = apply_act4<true>(acc0, a);
            out[ot1 * 64 + lane] = apply_act4<true>(acc1, a);
        } else {
            f32x4 acc = bp[(size_t)ot0 * 64 + lane];
            rew_glb_cf4* w0 = W + (size_t)ot0 * IT * 64 + lane;
#pragma unroll 4
            for (int it = 0; it < IT; ++it) {
                const f32x4 b = in[it * 64 + lane];
                const f32x4 a0 = w0[(size_t)it * 64];
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.x, b.x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.y, b.y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.z, b.z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a0.w, b.w, acc, 0, 0, 0);
            }
            out[ot0 * 64 + lane] = apply_act4<true>(acc, a);
        }
    }
}

// The Dense stack on the 16-row tile in xs (written and fenced by the caller).  Every thread of the workgroup calls it;
// thread tid < 16 gets row tid's reward, y * std_r + mean_r.  The caller's next write to xs comes behind the stack's
// barriers, so frames may call it in a loop without one of their own.
__device__ __forceinline__ float rew_mlp_stack(const RewMlpDesc& m, const RewMlpLds& lay, int tid) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int lane = tid & 63, wave = tid >> 6, nw = m.nw, L = m.n_layers;
    int in_off = lay.xs;
    for (int l = 0; l < L - 1; ++l) {
        const int out_off = (l & 1) ? lay.actB : lay.actA;
        rew_mlp_layer(m, l, in_off, out_off, wave, lane, nw);
        __syncthreads();
        in_off = out_off;
    }
    // the last layer: feature f of row p sits at tile_addr(f, p); partial j of row p takes f = j, j + J, ... in that order
    rew_lds_f* lds = (rew_lds_f*)smem;
    const rew_lds_f* in = lds + in_off;
    rew_lds_f* red = lds + lay.red;
    rew_glb_cf* wl = (rew_glb_cf*)m.wlast;
    const int K = m.dims[L - 1], p = tid & 15, j = tid >> 4, J = nw * 4;
    float acc = 0.0f;
    for (int f = j; f < K; f += J) acc = acc + in[tile_addr(f, p)] * wl[f];
    red[j * 16 + p] = acc;
    __syncthreads();
    float r = 0.0f;
    if (tid < 16) {
        float y = m.blast;
        for (int jj = 0; jj < J; ++jj) y = y + red[jj * 16 + tid];
        y = apply_act(y, m.act[L - 1]);
        r = m.normalized ? y * m.std_r + m.mean_r : y;
    }
    return r;
}

// input mean and std + 1e-7 (bbmpc_process_input's epsilon) to LDS, the input tile's padding to zero; ends with a barrier
__device__ __forceinline__ void rew_mlp_prologue(const RewMlpDesc& m, const RewMlpLds& lay, int tid, int nthr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* nmean = smem + lay.norm;
    float* nden = nmean + m.D;
    for (int f = tid; f < m.D; f += nthr) {
        nmean[f] = m.normalized ? m.mean_in[f] : 0.0f;
        nden[f] = m.normalized ? m.std_in[f] + 1e-7f : 1.0f;
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) smem[lay.xs + i] = 0.0f;
    __syncthreads();
}

// input column k of a row: which block it belongs to and the element inside it
__device__ __forceinline__ float rew_mlp_input(const RewMlpDesc& m, int k, const float* cur, const float* act, const float* nxt) {
    if ((m.mask & 1) && k < m.S) return cur[k];
    if ((m.mask & 2) && k < m.off_a + m.U) return act[k - m.off_a];
    return nxt[k - m.off_n];
}

__global__ void k_reward_mlp_traj(RewMlpTrajArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RewMlpDesc& m = q.m;
    const int tid = threadIdx.x, nthr = m.nw * 64;
    const int a = blockIdx.y, n0 = blockIdx.x * MLP_TP;
    const int t0 = blockIdx.z * q.tchunk, t1 = min(q.H, t0 + q.tchunk);
    const int S = m.S, U = m.U, D = m.D;
    const RewMlpLds lay = rew_mlp_lds_layout(m);
    float* xs = smem + lay.xs;
    const float* nmean = smem + lay.norm;
    const float* nden = nmean + D;
    rew_mlp_prologue(m, lay, tid, nthr);
    // a thread's first element i = tid of the 16 x D tile is row pp0, column k0 in every step: divided once.  With at least
    // 16 * D / 64 threads per element that is the only one (46 inputs on 13 waves: 736 elements, 832 threads); narrow
    // workgroups on wide inputs decompose their further elements in the loop
    const int pp0 = tid / D, k0 = tid - pp0 * D;
    for (int t = t0; t < t1; ++t) {
        for (int i = tid; i < MLP_TP * D; i += nthr) {             // a row's columns are consecutive threads: S contiguous floats of traj
            const int pp = i == tid ? pp0 : i / D, k = i == tid ? k0 : i - pp * D;
            const int n = n0 + pp;
            float v = 0.0f;
            if (n < q.n_pop) {
                if ((m.mask & 1) && k < S) {
                    v = t == 0 ? q.state[a * S + k] : q.traj[((((size_t)(t - 1) * q.A + a) * q.Nst) + n) * S + k];
                } else if ((m.mask & 2) && k < m.off_a + U) {
                    const int jj = t * U + (k - m.off_a);
                    v = q.from_ref ? q.seq[((size_t)n * q.A + a) * q.HU + jj] : q.cand[((size_t)a * q.HU + jj) * q.Nst + n];
                } else {
                    v = q.traj[((((size_t)t * q.A + a) * q.Nst) + n) * S + (k - m.off_n)];
                }
                v = (v - nmean[k]) / nden[k];                      // bbmpc_process_input: (x - mean) / (std + 1e-7)
            }
            xs[tile_addr(k, pp)] = v;
        }
        __syncthreads();
        const float r = rew_mlp_stack(m, lay, tid);
        if (tid < MLP_TP && n0 + tid < q.n_pop) q.step_out[((size_t)t * q.A + a) * q.Nst + n0 + tid] = r;
    }
}

// rewards[a][n] = (sum over t = 0 .. H-1, ascending, of step[t][a][n]; NaN -> -1e6) + rewards[a][n]   (deterministic.py:62-77;
// `rewards` holds -(penalty) from the rollout kernel, 0 without one)
__global__ void k_reward_mlp_finish(int n_pop, int A, int H, int Nst, const float* __restrict__ step, float* __restrict__ rewards) {
    const int a = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_pop) return;
    float total = 0.0f;
    for (int t = 0; t < H; ++t) total = total + step[((size_t)t * A + a) * Nst + n];
    if (total != total) total = -1.0e6f;
    rewards[(size_t)a * Nst + n] = total + rewards[(size_t)a * Nst + n];
}

__global__ void k_reward_mlp_rows(RewMlpRowsArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RewMlpDesc& m = q.m;
    const int tid = threadIdx.x, nthr = m.nw * 64;
    const int r0 = blockIdx.x * MLP_TP, D = m.D;
    const RewMlpLds lay = rew_mlp_lds_layout(m);
    float* xs = smem + lay.xs;
    const float* nmean = smem + lay.norm;
    const float* nden = nmean + D;
    rew_mlp_prologue(m, lay, tid, nthr);
    for (int i = tid; i < MLP_TP * D; i += nthr) {
        const int pp = i / D, k = i - pp * D, r = r0 + pp;
        float v = 0.0f;
        if (r < q.B) {
            const float* cur = (q.first && r % q.period == 0) ? q.first + (size_t)(r / q.period) * m.S
                                                              : q.cur + ((long)r - q.cur_shift) * q.cur_stride;
            v = rew_mlp_input(m, k, cur, q.act + (long)r * q.act_stride, q.nxt + (long)r * q.nxt_stride);
            v = (v - nmean[k]) / nden[k];
        }
        xs[tile_addr(k, pp)] = v;
    }
    __syncthreads();
    const float r = rew_mlp_stack(m, lay, tid);
    if (tid < MLP_TP && r0 + tid < q.B) q.out[r0 + tid] = r;
}

// rewards[a][n] = rewards[a][n] + w * V(s_H[n, a]); a NaN w * V makes the score -1e6.  Rows past
// n_pop are neither read nor written: their input columns stay zero.
__global__ void k_value_mlp_terminal(ValMlpTermArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const RewMlpDesc& m = q.m;
    const int tid = threadIdx.x, nthr = m.nw * 64;
    const int a = blockIdx.y, n0 = blockIdx.x * MLP_TP, D = m.D;
    const RewMlpLds lay = rew_mlp_lds_layout(m);
    float* xs = smem + lay.xs;
    const float* nmean = smem + lay.norm;
    const float* nden = nmean + D;
    rew_mlp_prologue(m, lay, tid, nthr);
    rew_glb_cf* last = (rew_glb_cf*)q.last + ((size_t)a * q.Nst + n0) * D;      // the tile's 16 rows are 16 * S contiguous floats
    for (int i = tid; i < MLP_TP * D; i += nthr) {
        const int pp = i / D, k = i - pp * D;
        float v = 0.0f;
        if (n0 + pp < q.n_pop) v = (last[i] - nmean[k]) / nden[k];
        xs[tile_addr(k, pp)] = v;
    }
    __syncthreads();
    const float v = rew_mlp_stack(m, lay, tid);
    if (tid < MLP_TP && n0 + tid < q.n_pop) {
        const size_t o = (size_t)a * q.Nst + n0 + tid;
        const float term = q.weight * v;
        float total = q.rewards[o] + term;
        if (term != term) total = -1.0e6f;
        q.rewards[o] = total;
    }
}

#endif  // BBMPC_TU_MLP

}  // namespace bbmpc
