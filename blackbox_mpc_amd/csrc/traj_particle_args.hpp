// The arguments every trajectory-distribution kernel takes (bbmpc_predict_trajectory_particles; the semantics are in
// kernels_traj_particles.hpp).  A header of its own so that the bbmpc_mlp unit, which launches the learned model's kernel
// (kernels_mlp_traj_particles.hpp), does not compile the pendulum and moment kernels it never launches.
#pragma once

namespace bbmpc {

struct TrajParticleArgs {
    int B, P, Hq, U, S;
    int reward_kind, fix_q1;
    const float* states;      // [B, S]
    const float* seq;         // [B, Hq, U]
    const float* sigma;       // [S] process noise standard deviation
    const float* eps;         // [B][P][Hq][S] standard normals
    float* pstates;           // [B][P][Hq][S]   (never null: the caller's tensor or the handle's scratch)
    float* prewards;          // [B][P][Hq]
};

}  // namespace bbmpc
