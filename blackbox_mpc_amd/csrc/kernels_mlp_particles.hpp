// Particle rollouts through the learned model (kernels_particles.hpp has the semantics): the frame of k_traj_mlp
// (kernels_mlp_traj.hpp) -- 16 rows per workgroup, the generic MFMA recurrence of kernels_mlp.hpp (SPEC 0:
// v_mfma_f32_16x16x4_f32, packed wp4 operands, run-time activation codes), the state tile resident in LDS, the next step's
// actions fetched while the Dense stack runs -- with rows that are (candidate, particle) pairs of ONE agent (grid.y = agent,
// a tile mixes candidates and two rows share an action only when they share the candidate):
//   - every row starts from the agent's state;
//   - the step's noise elements are fetched in front of the Dense stack, held in registers across it and added in the
//     epilogue, so the noisy state is what the reward and the next step see;
//   - the reward is summed per row in a register of wave 0's first 16 lanes; nothing is stored per step, the NaN rule and
//     one store per row close the kernel.
// One kernel text, k_rollout_mlp_particles_kind<ARGS, EXT>, instantiated directly on the argument struct of each of its
// three kinds.  Profiles tell the kinds apart by ARGS, bbmpc_get_profile by the names in the second column:
//   MlpParticleArgs       k_rollout_mlp_particles        one model: grid (ceil(n_pop * P / 16), A), row r = n * P + p;
//   MlpEnsParticleArgs    k_rollout_mlp_particles_ens    a bootstrap ensemble with trajectory sampling (DESIGN.md section
//       8c), particle p of every candidate follows member p % E for the whole horizon.  An MFMA tile multiplies ONE set of
//       weights, so a tile must be uniform in the member: grid (ceil(n_pop * Pe / 16), A, E), Pe = P / E (the host refuses
//       P % E != 0), row r of member e = blockIdx.z is candidate r / Pe, particle e + E * (r % Pe), on the operands
//       kernels_mlp_ensemble.hpp describes;
//   MlpGaussParticleArgs  k_rollout_mlp_particles_gauss  log-variance heads (DESIGN.md section 8d,
//       kernels_mlp_gaussian.hpp) on the ensemble's row space; without an ensemble E = 1 with the primary's operands and
//       stride 0.
// Every instantiation compiles to the instruction stream the three separate kernels had; the order of the statements below
// is theirs, and reordering them moves instructions.
// A third template argument, TRAJ, gives the form a HIP-source reward needs: no reward and no returns
// store, instead every step's noisy next states go to ParticleArgs::traj, feature-major [H][A][S][RS], for rtc.hpp's
// bbmpc_user_reward_particles to score.  Everything TRAJ adds is behind `if constexpr`: the TRAJ = false instantiations are
// the kernels they were (same resource remarks).
// Dims, activations and the normalisation statistics are the primary model's (MlpDesc).  Offsets into the action source and
// the noise are 32 bit (the host refuses larger buffers).
// The prologue and the epilogue restate k_traj_mlp / rollout_mlp_body<0>: a fix in one of them belongs here as well.
// Compiled in the bbmpc_mlp unit only.
#pragma once
#include "kernels_mlp_traj.hpp"
#include "kernels_mlp_ensemble.hpp"
#include "kernels_mlp_gaussian.hpp"
#include "kernels_particles.hpp"

namespace bbmpc {

enum MlpParticleKind { MLP_PART_PLAIN = 0, MLP_PART_ENS = 1, MLP_PART_GAUSS = 2 };

// One argument struct per kind (ARGS::KIND selects the kind at compile time): the single-model kind carries no member or
// head field.
struct MlpParticleArgs {
    static constexpr int KIND = MLP_PART_PLAIN;
    MlpDesc m;
    const float* wp4[MLP_MAX_LAYERS];    // MlpRolloutArgs::wp4
    int nw;                              // waves per workgroup
    ParticleArgs p;
};

struct MlpEnsParticleArgs {
    static constexpr int KIND = MLP_PART_ENS;
    MlpDesc m;                           // the primary's dims / activations / statistics; bpack = member 0's packed biases
    const float* wp4[MLP_MAX_LAYERS];    // member 0's packed operands (MlpRolloutArgs::wp4's layout)
    int wstride[MLP_MAX_LAYERS];         // floats between two members' operands of a layer
    int bstride[MLP_MAX_LAYERS];         // ... and between their packed biases
    int nw;                              // waves per workgroup
    int E;                               // members
    ParticleArgs p;
};

struct MlpGaussParticleArgs {
    static constexpr int KIND = MLP_PART_GAUSS;
    MlpDesc m;                           // the primary's dims / activations / statistics; bpack = member 0's packed biases
    const float* wp4[MLP_MAX_LAYERS];    // member 0's packed operands (MlpRolloutArgs::wp4's layout)
    int wstride[MLP_MAX_LAYERS];         // floats between two members' operands of a layer (0 without an ensemble)
    int bstride[MLP_MAX_LAYERS];         // ... and between their packed biases
    const float* hp4;                    // head 0's packed operands, the last layer's layout [OT][IT][64][4]
    const float* hbp;                    // head 0's packed biases [OT][64][4]
    int hwstride, hbstride;              // floats between two heads
    const float* min_logvar;             // [S]
    const float* max_logvar;             // [S]
    int nw;                              // waves per workgroup
    int E;                               // members (1 without an ensemble)
    ParticleArgs p;
};

constexpr int MLP_PART_ROWSLOT = MLP_TP;      // TRAJ: ints behind the layout's total
constexpr int MLP_PART_PF = 2;      // noise elements a thread holds in registers across a step's Dense stack

template <class ARGS, bool EXT, bool TRAJ = false>
__global__ void k_rollout_mlp_particles_kind(ARGS q) {
    constexpr int KIND = ARGS::KIND;
    constexpr bool MEMBER = KIND != MLP_PART_PLAIN;       // rows grouped by member, grid.z = member
    constexpr bool GAUSS = KIND == MLP_PART_GAUSS;        // a log-variance head behind the last layer
    // noise elements held in registers across the Dense stack.  The head's TRAJ form is the one instantiation at the register
    // limit with nothing to give: it holds one (the others are fetched in the epilogue, which only networks of fewer than
    // 16 * S / 64 waves notice) and so stays free of scratch.
    constexpr int NPF = (TRAJ && GAUSS) ? 1 : MLP_PART_PF;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const MlpDesc& m = q.m;
    const ParticleArgs& pa = q.p;
    const int a = blockIdx.y;
    const int e = MEMBER ? (int)blockIdx.z : 0;           // the member of every row of this workgroup
    const int n0 = blockIdx.x * MLP_TP;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = q.nw, nthr = nw * 64;
    const int S = pa.S, U = pa.U, H = pa.H, L = m.n_layers, P = pa.P;
    // ---- the row map: row r of this workgroup's (agent, member) -> candidate, particle; the store that closes the kernel turns
    // them into the element of the agent's returns.  With members the rows of member e walk its particles e, e + E, ... of
    // candidate 0, then candidate 1's.  Its scalars are read here, in front of the LDS layout, and its functions follow the
    // LDS pointers: the statement order of this kernel decides the instruction order, and this one is measured.
    int E = 1, Pe = P;                          // members, particles per member
    if constexpr (MEMBER) {
        E = q.E;
        Pe = P / E;
    }
    const int R = pa.n_pop * Pe;                // rows of this (agent, member)
    const int Sp = (S + 3) & ~3;
    const MlpTrajLds lay = GAUSS ? mlp_gauss_lds_layout(m, U, S, nw) : mlp_traj_lds_layout(m, U, S, nw);
    float* xs = smem + lay.xs;
    float* part = smem + lay.part;
    float* st = smem + lay.st;
    float* acts = smem + lay.acts;
    const bool normd = m.normalized != 0;
    float* nmean = smem + lay.norm;             // [S+U] input means (0 when not normalised)
    float* ninv = nmean + (S + U);              // [S+U] 1/(std + 1e-7)   (1 when not normalised)
    float* tmean = ninv + (S + U);              // [S] target mean
    float* tstd = tmean + S;                    // [S] target std + 1e-7
    float* lbias = tstd + S;                    // [S] bias of the last layer
    float* hbias = lbias + S;                   // GAUSS: [S] bias of the log-variance head
    float* minlv = hbias + S;                   // GAUSS: [S] bounds of the soft clamp
    float* maxlv = minlv + S;

    // ---- the row map's functions
    auto row_n = [&](int r) -> int { return r / Pe; };
    auto row_p = [&](int r) -> int {
        if constexpr (MEMBER) return e + E * (r % Pe);
        else return r % Pe;
    };
    // ---- the operands and packed biases of layer l
    auto layer_w = [&](int l) -> const float* {
        if constexpr (MEMBER) return q.wp4[l] + e * q.wstride[l];
        else return q.wp4[l];
    };
    auto layer_b = [&](int l) -> const float* {
        if constexpr (MEMBER) return m.bpack[l] + e * q.bstride[l];
        else return m.bpack[l];
    };
    // ---- what a fetched noise element is: sigma[f] * eps, or eps alone where the scale is known only behind the Dense stack
    auto noise_elem = [&](float sig, float eps) -> float {
        if constexpr (GAUSS) return eps;
        else return sig * eps;
    };

    // what this thread fetches every step, fixed across the horizon: action elements el = tid + j * nthr of the tile
    // [16][U] (offset of step 0 and the distance between steps, -1 = none) and noise elements i = tid + j * nthr of the
    // tile [S][16] (offset of step 0 in pnoise, -1 = a row past the last).  32-bit offsets: the host refuses larger buffers.
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
    int nbase[NPF];
    float nsig[NPF];
#pragma unroll
    for (int j = 0; j < NPF; ++j) {
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
        return noise_elem(pa.sigma[f], pa.pnoise[(((size_t)a * P + row_p(n0 + pp)) * H + t) * S + f]);
    };

    for (int f = tid; f < S + U; f += nthr) {
        const float mu = normd ? (f < S ? m.mean_s[f] : m.mean_a[f - S]) : 0.0f;
        const float sd = normd ? (f < S ? m.std_s[f] : m.std_a[f - S]) : 1.0f;
        nmean[f] = mu;
        ninv[f] = normd ? 1.0f / (sd + 1e-7f) : 1.0f;          // system_dynamics_handler.py:119-122 (x - mu)/(sd + 1e-7)
        if (f < S) {
            tmean[f] = normd ? m.mean_t[f] : 0.0f;
            tstd[f] = normd ? (m.std_t[f] + 1e-7f) : 1.0f;
            const size_t bslot = ((size_t)(f >> 4) * 64 + ((f & 15) >> 2) * 16) * 4 + (f & 3);     // feature f in [OT][64][4]
            lbias[f] = layer_b(L - 1)[bslot];
            if constexpr (GAUSS) {
                hbias[f] = (q.hbp + e * q.hbstride)[bslot];
                minlv[f] = q.min_logvar[f];
                maxlv[f] = q.max_logvar[f];
            }
        }
    }
    for (int i = tid; i < m.tiles[0] * 256; i += nthr) xs[i] = 0.0f;
    for (int i = tid; i < MLP_TP * S; i += nthr) {                 // tf.tile(current_states, ...): every row, the agent's state
        const int pp = i / S, s = i % S;
        st[pp * Sp + s] = pa.state[(size_t)a * S + s];
    }
    for (int el = tid; el < MLP_TP * U; el += nthr) acts[el] = fetch_action(el, 0);     // (rows past the last roll zeros)
    __syncthreads();
    for (int i = tid; i < MLP_TP * (S + U); i += nthr) {          // normalised layer-0 input for t = 0
        const int f = i / MLP_TP, pp = i % MLP_TP;
        const float v = (f < S) ? st[pp * Sp + f] : acts[pp * U + (f - S)];
        xs[tile_addr(f, pp)] = (v - nmean[f]) * ninv[f];
    }
    __syncthreads();

    const int OTl = m.tiles[L];
    float racc = 0.0f;                                 // lanes 0..15 of wave 0: the row's reward sum
    // TRAJ: the slot of each of the tile's rows in a feature's run of pa.traj -- its returns index, -1 = a row past the last --
    // in the MLP_PART_ROWSLOT ints the launch adds behind the layout (as k_traj_mlp_particles_kind keeps its row map: a
    // register held across the Dense stack spills in the widest instantiation).  Published by the barriers of step 0.
    [[maybe_unused]] int* rowslot = reinterpret_cast<int*>(smem + lay.total);
    if constexpr (TRAJ) {
        if (tid < MLP_TP) rowslot[tid] = (n0 + tid < R) ? (MEMBER ? row_n(n0 + tid) * P + row_p(n0 + tid) : n0 + tid) : -1;
    }
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
        float en[NPF];
#pragma unroll
        for (int j = 0; j < NPF; ++j) en[j] = nbase[j] >= 0 ? noise_elem(nsig[j], pa.pnoise[nbase[j] + t * S]) : 0.0f;
        // ---- dense layers (kernels_mlp.hpp, SPEC 0)
        int in_off = lay.xs;
        for (int l = 0; l < L - 1; ++l) {
            const int out_off = (l & 1) ? lay.actB : lay.actA;
            if constexpr (MEMBER) mlp_layer_out_split_member<EXT>(m, layer_w(l), layer_b(l), l, in_off, out_off, wave, lane, nw);
            else mlp_layer_out_split<EXT>(m, layer_w(l), l, in_off, out_off, wave, lane, nw);
            __syncthreads();
            in_off = out_off;
        }
        if constexpr (GAUSS) mlp_layer_k_split_gauss(m, layer_w(L - 1), q.hp4 + e * q.hwstride, L - 1, in_off, lay.part, wave, lane, nw);
        else mlp_layer_k_split(m, layer_w(L - 1), L - 1, in_off, lay.part, wave, lane, nw);
        __syncthreads();
        // ---- epilogue: reduce partials (GAUSS: the head's too), bias, last activation (mean only), de-normalise, residual,
        // NOISE (GAUSS: scaled here); stage step t + 1's input.  `d` is a noise_elem, `sig` its sigma[f] (read by GAUSS only).
        const int nwp = min(nw, m.tiles[L - 1]);          // waves that actually produced partials
        auto epilogue = [&](int i, float sig, float d) {
            const int f = i / MLP_TP, pp = i % MLP_TP;
            const int ot = f >> 4, ln = ((f & 15) >> 2) * 16 + pp, rg = f & 3;
            const float* pp0 = part + (((size_t)ot) * 64 + ln) * 4 + rg;
            [[maybe_unused]] const float* hp0 = pp0 + (size_t)nw * OTl * 256;       // GAUSS: the head's partials lie behind the mean's
            float acc = lbias[f];
            for (int w = 0; w < nwp; ++w) acc = acc + pp0[(size_t)w * OTl * 256];
            float z = 0.0f;
            if constexpr (GAUSS) {
                z = hbias[f];
                for (int w = 0; w < nwp; ++w) z = z + hp0[(size_t)w * OTl * 256];
            }
            acc = apply_act_rt<EXT>(acc, m.act[L - 1]);                     // (the head has no activation)
            const float dev = normd ? tmean[f] + acc * tstd[f] : acc;       // system_dynamics_handler.py:152-155
            if constexpr (GAUSS) {
                const float lv1 = maxlv[f] - bb_softplusf(maxlv[f] - z);    // PETS' soft clamp of the log-variance
                const float lv = minlv[f] + bb_softplusf(lv1 - minlv[f]);
                const float sd = tstd[f] * bb_exp_rel(0.5f * lv);           // (tstd is 1 when not normalised)
                d = (sig + sd) * d;
            }
            const float ns = (dev + cur[pp * Sp + f]) + d;                  // transforms.py:34, + sigma * eps / (sigma + sd) * eps
            nxt[pp * Sp + f] = ns;
            xs[tile_addr(f, pp)] = (ns - nmean[f]) * ninv[f];
        };
#pragma unroll
        for (int j = 0; j < NPF; ++j) {
            const int i = tid + j * nthr;
            if (i < MLP_TP * S) epilogue(i, nsig[j], en[j]);
        }
        for (int i = tid + NPF * nthr; i < MLP_TP * S; i += nthr) epilogue(i, pa.sigma[i / MLP_TP], fetch_noise(i, t));
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
        if constexpr (TRAJ) {
            // no reward here (the kind is REW_NONE): the step's noisy next states go to pa.traj [H][A][S][RS] instead, from
            // the LDS tile and BEHIND the barrier, so the stores drain under step t + 1's Dense stack and no barrier the
            // MFMA loop waits on has them in front of it.  16 consecutive lanes write 16 consecutive rows of one feature
            // (64 bytes; with members the slots of one candidate are E apart).  `nxt` is next written by step t + 2's epilogue.
            const int pp = tid & (MLP_TP - 1);       // every element i = tid + j * nthr of this thread is of row tid % 16
            const int slot = rowslot[pp];
            if (slot >= 0) {
#pragma unroll 1
                for (int i = tid; i < MLP_TP * S; i += nthr) {
                    const int f = i / MLP_TP;
                    pa.traj[((t * pa.A + a) * S + f) * pa.RS + slot] = nxt[pp * Sp + f];
                }
            }
        } else if (tid < MLP_TP)
            racc = racc + reward_generic(pa.reward_kind, pa.fix_q1 != 0, cur + tid * Sp, act_t + tid * U, nxt + tid * Sp, S, U);
    }
    if constexpr (TRAJ) return;                                 // (the scorer writes the returns: rtc.hpp bbmpc_user_reward_particles)
    if (tid < MLP_TP && n0 + tid < R) {
        if (racc != racc) racc = -1.0e6f;                       // deterministic.py:75-77, per particle
        // the row's element of the agent's returns, n * P + p (without members the row itself; two index expressions here, not
        // one in the row map, because the address is formed from the expression's shape and a helper moves instructions)
        if constexpr (MEMBER) pa.returns[(size_t)a * pa.RS + (size_t)row_n(n0 + tid) * P + row_p(n0 + tid)] = racc;
        else pa.returns[(size_t)a * pa.RS + n0 + tid] = racc;
    }
}

}  // namespace bbmpc
