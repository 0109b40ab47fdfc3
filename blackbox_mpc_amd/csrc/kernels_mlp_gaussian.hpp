// What PROBABILISTIC learned models (bbmpc_set_mlp_logvar_head) add to the particle rollout frame of
// kernels_mlp_particles.hpp.  Every model -- the handle's, or each member of its ensemble -- carries a log-variance head, a
// second last Dense layer on the last hidden activation, and the noise scale of a step becomes state dependent:
//     nxt = predict_next_state_member(s_t, a_t) + (sigma[f] + sd_f(s_t, a_t)) * eps[a, p, t, f]
//     z = h W_v + b_v;  lv1 = max_lv - softplus(max_lv - z);  lv = min_lv + softplus(lv1 - min_lv);  sd = tstd * exp(lv / 2)
// The last layer multiplies the input tile into the mean's output tiles and into the head's (packed by mlp_pack_layer like
// the mean's, [OT][IT][64][4] per member): two independent accumulator chains per k tile, the mean's in the order
// mlp_layer_k_split runs them, so the mean has the bits the frame gives without heads.  The head's partial sums lie behind
// the mean's in LDS (mlp_gauss_lds_layout: `part` doubled, three more [S] vectors in `norm`).
// Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_traj.hpp"

namespace bbmpc {

constexpr float MLP_LOGVAR_ABS_MAX = 40.0f;      // |min_logvar|, |max_logvar| <= 40: exp(lv / 2) stays far inside fp32

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

}  // namespace bbmpc
