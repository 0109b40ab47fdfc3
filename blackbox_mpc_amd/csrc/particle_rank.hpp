// Stable rank of P <= 64 values held one per lane of a wave:
//     rank[p] = #{q : x[q] < x[p]} + #{q < p : x[q] == x[p]}
// The ranks of lanes 0 .. P-1 are 0 .. P-1, each exactly once; equal values are ordered by lane.  Every comparison is
// exact, so the selection that follows a rank (the CVaR tail of kernels_particles.hpp, the nearest-rank quantiles of
// kernels_traj_particles.hpp) is exact given the bits of x.  Lane p loops over the wave-uniform broadcasts of x[0 .. P)
// and counts: P iterations, no LDS, no scratch, no dynamic register indexing.  A NaN compares false everywhere: it counts
// nothing and is counted by nobody, so the ranks are then no permutation and mean nothing -- callers that can see a NaN
// say so in their own contract (the returns the CVaR score ranks are NaN-free: NaN -> -1e6 per particle).
#pragma once
#include <hip/hip_runtime.h>

namespace bbmpc {

// x of lane j (j wave-uniform) in every lane
__device__ __forceinline__ float wave_bcast(float x, int j) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), j));
}

// Call with all 64 lanes of the wave active; lanes >= P hold anything and get a rank that means nothing.
__device__ __forceinline__ int particle_stable_rank(float x, int lane, int P) {
    int rank = 0;
    for (int j = 0; j < P; ++j) {
        const float xj = wave_bcast(x, j);
        rank += (xj < x || (xj == x && j < lane)) ? 1 : 0;
    }
    return rank;
}

}  // namespace bbmpc
