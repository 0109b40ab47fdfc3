// What a bootstrap ENSEMBLE of learned models (bbmpc_set_mlp_ensemble) adds to the particle rollout
// frame of kernels_mlp_particles.hpp: the hidden layer on a member's operands.  The members' packed operands
// [OT][IT][64][4] and biases [OT][64][4] of a layer lie one behind the other at a fixed stride; the frame adds
// member * stride to the base pointers, uniform per workgroup (scalar registers, no pointer table).
// Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_traj.hpp"

namespace bbmpc {

constexpr int MLP_ENS_MAX = 8;           // members of an ensemble

// mlp_layer_out_split (kernels_mlp.hpp; the measurements behind its shape are written there) with the layer's packed biases
// passed in, where that one reads m.bpack[l]: the member's, at the same [OT][64][4] layout.  Statement for statement the
// same arithmetic, so a member equal to the primary gives the primary's bits.
// A copy, because a bias parameter on mlp_layer_out_split itself moved instructions in the generic kernels that share it.
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

}  // namespace bbmpc
