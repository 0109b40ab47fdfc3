// Where the persistent pendulum kernel's prefetched-draws rollout (kernels_fused.hpp, INJ == 2) reads in the buffer
// k_noise_fill writes, for the kernel's addressing and the host's allocation alike: plain C++, no HIP needed.
//
// Layout: [step][it][A][Nst][Q] float4, Q = ceil(H / 4) (U == 1); one float4 = one Philox block = the draws of 4 model steps
// of one trajectory.  A trajectory's row is its Q consecutive float4.  The rollout loads its draws two blocks ahead of
// their use through a pointer that walks the row, with no clamp: behind the last block it needs it goes on reading up to
// two float4 PAST THE ROW'S END.  Those land in the next trajectory's row (the next agent's, iteration's, control step's
// first row behind the last one) or, behind the last row of a chunk buffer, in the pad the host allocates behind it.
// None of them ever reaches a result: the blocks a model step uses are 0 .. Q - 1.
#pragma once
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BBMPC_NOISE_HD __host__ __device__ __forceinline__
#else
#define BBMPC_NOISE_HD inline
#endif

namespace bbmpc {

// float4 index of trajectory n's first Philox block within one control step's draws
BBMPC_NOISE_HD size_t noise_block_index(int it, int A, int a, int Nst, int n, int Q) {
    return (((size_t)it * A + a) * Nst + n) * Q;
}

// The highest block of its row (0 = the row's first float4) a trajectory's rollout loads.
//  CEM / PI2 / RandomSearch: blocks 0 and 1 up front, then blocks b + 2 and b + 3 in every trip b = 0, 2, 4, ... that
//  starts with two whole blocks ahead (b + 1 < H / 4); the single block and the remainder steps behind the trips load nothing.
//  SPSA: block 0 up front, block b + 1 while block b < Q runs.
BBMPC_NOISE_HD int noise_last_block_read(int H, bool spsa) {
    const int nblk = H >> 2, Q = (H + 3) >> 2;
    return spsa ? Q : (nblk & ~1) + 1;
}

// float4 past the end of its row that the rollout may load (0, 1 or 2): what an allocation has to hold behind its last row
BBMPC_NOISE_HD int noise_pad_blocks(int H) {
    const int Q = (H + 3) >> 2;
    const int a = noise_last_block_read(H, false), b = noise_last_block_read(H, true);
    return (a > b ? a : b) - (Q - 1);
}

// the highest float4 index, within one control step's draws, that trajectory n of agent a loads in iteration `it`
BBMPC_NOISE_HD size_t noise_extent_index(int it, int A, int a, int Nst, int n, int Q, int H, bool spsa = false) {
    return noise_block_index(it, A, a, Nst, n, Q) + (size_t)noise_last_block_read(H, spsa);
}

// floats of one control step's draws, of the pad, and of a chunk buffer of `steps` control steps with its pad.  (The pad is
// not part of a chunk: the resident kernel's prediction of the next request's pointer compares against the unpadded size.)
BBMPC_NOISE_HD size_t noise_step_floats(int iters, int A, int Nst, int H) { return (size_t)iters * A * Nst * ((H + 3) >> 2) * 4; }
BBMPC_NOISE_HD size_t noise_pad_floats(int H) { return (size_t)noise_pad_blocks(H) * 4; }
BBMPC_NOISE_HD size_t noise_alloc_floats(int steps, int iters, int A, int Nst, int H) {
    return noise_step_floats(iters, A, Nst, H) * (size_t)steps + noise_pad_floats(H);
}

}  // namespace bbmpc
