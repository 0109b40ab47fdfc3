// Persistent per-control-step kernel for the analytic (true-model) path.
//
// One workgroup owns one agent for the WHOLE control step: distribution init, every optimizer
// iteration (sample -> H-step rollout -> reward -> top-k / softmin / argmax -> refit) and the
// OptimizerBase.__call__ tail (exploration noise, predicted next state + reward) run inside a single
// launch, synchronised only by workgroup barriers.  Nothing but the [A,S] state comes in and the
// packed [A,U+S+1] record goes out; rewards, the sampling distribution and (when they fit) the
// candidate action sequences live in LDS, so an optimizer iteration moves no HBM traffic at all.
//
// Replaces, per control step, what the reference executes as one tf.function graph:
//   OptimizerBase.__call__ (optimizer_base.py:55-95) -> {CEM,PI2,RandomSearch}._optimize
//   (cem.py:74-136, pi2.py:58-96, random_search.py:38-48) -> DeterministicTrajectoryEvaluator.__call__
//   (deterministic.py:26-77) -> PendulumTrueModel / pendulum_reward_function (utils/pendulum.py).
#pragma once
#include <type_traits>

#include "kernels_opt.hpp"
#include "kernels_refit.hpp"
#include "kernels_rollout.hpp"
#include "noise_extent.hpp"
#include "topk.hpp"

namespace bbmpc {

constexpr int FOPT_RS = 1;
constexpr int FOPT_CEM = 2;
constexpr int FOPT_PI2 = 3;
constexpr int FOPT_SPSA = 4;
constexpr int FUSED_MAX_SPSA_ITERS = 16;

struct FusedArgs {
    int N, A, H, U, HU, Nst, k, iters;
    int agent_offset;
    int fix_q1, fix_q7, add_noise;
    int warm_start;          // CEM: BBMPC_FIX_Q2 (keep the mean across control steps)
    unsigned* done_flag;     // optional completion counter in signal memory (see the kernel's tail), else null;
                             // LINGER: [A][16] pinned completion lines, which carry the records (p.record is not written)
    unsigned* done_count;
    unsigned done_value;
    float alpha, inv_lamda;
    const float* state;      // [A,3]
    const float* lo;
    const float* hi;
    float* prev_mean;        // [A][HU] in/out (warm start)
    const float* var0;       // [A][HU]
    float* mean_out;         // [A][HU] last mean (get_state)
    float* var_out;          // [A][HU]
    float* samples_g;        // [A][HU][Nst] global scratch when the samples do not fit in LDS
    const float* inj;        // standard noise or null: INJ=1 caller-injected [iters][A][HU][Nst];
                             // INJ=2 prefetched by k_noise_fill, [iters][A][Nst][Q] float4 (particle-major Philox blocks)
    const float* inj_expl;   // injected exploration noise [A,U] or null
    float* record;           // [A][U+S+1]
    float* next_state;       // optional contiguous [A,S]
    // traces (null when disabled): [iters][A][Nst], [iters][A][HU], [iters][A][HU], [iters][A][k], [iters][A][HU][Nst]
    float spsa_ak[FUSED_MAX_SPSA_ITERS], spsa_ck[FUSED_MAX_SPSA_ITERS];   // SPSA gain sequences (spsa.py:69-70), per iteration
    float* t_rewards2;       // SPSA trace: rewards of the minus candidates [iters][A][Nst]
    float* t_rewards;
    float* t_mean;
    float* t_var;
    int* t_elites;
    float* t_samples;
    long long* dbg;          // optional phase clocks (debug)
    RngKey key;
    // LINGER variant (one agent, host-in / host-out calls): after publishing its record the workgroup stays on the GPU and
    // polls a 64-byte request line in pinned host memory for the next control step (see the end of the kernel)
    // Every agent's workgroup is on its own: a request line, a completion word and an exit word per agent (one cache line
    // each, arrays indexed by the agent), so no two workgroups ever have to agree on anything.
    const unsigned* mbox;    // [A][16] words: [0] = [15] = sequence number, [1] step, [2] add_noise, [3..4] noise pointer, [5..7] state
    unsigned* gone;          // [A][16] pinned words: the last sequence number handled, written when the workgroup leaves
    unsigned linger_ticks;   // how long to wait for a request, in wall_clock64 ticks (100 MHz)
    int test_quit_agent;     // test hook (BBMPC_LINGER_TEST_QUIT = a + 1): agent a's workgroup leaves after every control step, -1 = none;
                             // 1000 + a: every agent from a on leaves (more than one 16-entry line of the agent map)
    const int* amap;         // optional: blockIdx.x -> agent (a launch for a subset of the agents), null = identity
    // (LINGER, INJ = 2) the two noise chunk buffers and their strides: a resident workgroup fetches the first draws of the
    // NEXT control step while it waits for the request, from inj + pf_step_floats when that still lies inside the chunk
    // buffer inj lies in.  Timing only: the request names the pointer, and a fetch from anywhere else is thrown away.
    const float* pf_buf[2];
    unsigned long long pf_step_floats, pf_chunk_floats;      // floats per control step / per chunk buffer (0 = no prediction)
    int* t_passes;           // trace, with t_elites: [iters][A] radix passes of the elite selection (last: no other field moves)
    int wave_select;         // 512-thread CEM form: the selection may take the all-wave route (BBMPC_CEM_WAVE_SELECT=0 at handle creation: 0)
};

// (noise_block_index: the float4 index of particle n's first Philox block in the layout k_noise_fill writes,
// [it][A][Nst][Q], and how far behind it the rollout reads: noise_extent.hpp)

// phase clocks for kernel development: build with -DBBMPC_KERNEL_DBG and run with BBMPC_DBG=1
#ifdef BBMPC_KERNEL_DBG
#define BB_DBG(slot) do { if (p.dbg && tid == 0 && a == 0) dbg_lds[(slot)] = (long long)wall_clock64(); } while (0)
#else
#define BB_DBG(slot) do {} while (0)
#endif

__device__ __forceinline__ float block_min(float v, float* red, int tid, int nw) {
    v = wave_min(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = red[(tid & 63) < nw ? (tid & 63) : 0];
    r = wave_min(r);
    __syncthreads();
    return r;
}
__device__ __forceinline__ float block_sum(float v, float* red, int tid, int nw) {
    v = wave_sum(v);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    float r = ((tid & 63) < nw) ? red[tid & 63] : 0.0f;
    r = wave_sum(r);
    __syncthreads();
    return r;
}

// LDS carve (4-byte words): rewards[Nst] | mean[HUp] | var[HUp] | sigma[HUp] | eidx[kp] | red[64] | hist[..]  |
//                            ekeys[2*kp] | samples[HU][Nst]      (every piece a multiple of 16 B; hist = TOPK_HIST_WORDS)
// INVARIANT (the INJ == 2 rollout rests on it): mean[] and sigma[] are each FOLLOWED by at least 16 bytes of this carve.
// With H a multiple of four the rollout reads one float4 past mean[HUp] and past sigma[HUp] -- here: var[0..3] and
// eidx[0..3] (kp >= 4) -- and never uses it.  Whoever reorders the carve keeps a piece behind both, or pads them by a block
// (and Engine::optimize_fused's lds_base with them).
// 1: the 512-thread CEM form selects on the all-wave route where it applies (topk.hpp, block_topk_wave_select); 0 compiles
// today's route only.
#ifndef BBMPC_CEM_WAVE_SELECT
#define BBMPC_CEM_WAVE_SELECT 1
#endif
#ifndef BBMPC_FUSED_ACTIONS_AHEAD
#define BBMPC_FUSED_ACTIONS_AHEAD 1
#endif
// 0: the 512-thread CEM form runs its tail behind the last statistics barrier like every other form (A/B builds)
#ifndef BBMPC_FUSED_EARLY_TAIL
#define BBMPC_FUSED_EARLY_TAIL 1
#endif
// MAXT: the largest workgroup an instantiation may be launched with (its launch bound, hence its register budget: 1024
// threads leave a wave 128 VGPRs, 512 threads 256 at the same two waves per SIMD).  Engine::optimize_fused's launch_fused4
// is the one place that picks it.
template <int OPT, bool SAMPLES_LDS, bool FASTM, int INJ, int ILP, int MAXT = 1024, bool LINGER = false>
__global__ __launch_bounds__(MAXT) void k_fused_pendulum(FusedArgs p) {
    static_assert(MAXT == 512 || MAXT == 1024, "k_fused_pendulum: a launch bound of 512 or 1024 threads");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int a = p.amap ? p.amap[blockIdx.x] : (int)blockIdx.x;
    const int tid = threadIdx.x;
    const int nthr = blockDim.x;
    const int nw = nthr >> 6;
    const int HUp = (p.HU + 3) & ~3;
    const int kp = (p.k + 3) & ~3;
    float* rew = smem;
    float* mean = rew + p.Nst;
    float* var = mean + HUp;
    float* sigma = var + HUp;
    int* eidx = (int*)(sigma + HUp);
    float* red = (float*)(eidx + kp);
    uint32_t* hist = (uint32_t*)(red + 64);
    // (only CEM selects: the other optimizers keep the narrow words, i.e. the carve they always had)
    unsigned long long* ekeys = (unsigned long long*)(hist + (OPT == FOPT_CEM ? TOPK_HIST_WORDS : TOPK_HIST_WORDS_NARROW));
    float* samp = SAMPLES_LDS ? (float*)(ekeys + kp) : (p.samples_g + (size_t)a * p.HU * p.Nst);
    // the all-wave selection: the 512-thread CEM form only.  Its prepass keeps the per-wave (kmin, bound) slots in red[0..8)
    // and red[32..40), which the CEM form uses for nothing else (red[16..31]: the request's words, red[60..62]: the state),
    // and zeroes the second histogram itself (topk.hpp).
    constexpr bool WAVE_SEL = BBMPC_CEM_WAVE_SELECT && OPT == FOPT_CEM && MAXT == 512 && SAMPLES_LDS;
    [[maybe_unused]] uint32_t* const slot_min = (uint32_t*)red;
    [[maybe_unused]] uint32_t* const slot_bound = (uint32_t*)red + 32;
#ifdef BBMPC_KERNEL_DBG
    __shared__ long long dbg_lds[48];
#endif
    const PendulumModel model{p.fix_q1 != 0};
    const float lo = p.lo[0], hi = p.hi[0];
    // what changes from one control step to the next (the LINGER variant serves several per launch)
    RngKey key_s = p.key;
    const float* inj_s = p.inj;
    int add_noise_s = p.add_noise;
    unsigned done_value_s = p.done_value;
    // the [A,3] state may live in pinned host memory (bbmpc_optimize's zero-copy path): three lanes fetch it -- one PCIe
    // read per workgroup instead of three per wave (3072 at 64 agents x 16 waves) -- and LDS hands it to everybody
    if (tid < 3) red[60 + tid] = p.state[a * 3 + tid];
    // a resident kernel keeps the next control step's starting distribution in registers (CEM: the same restart mean /
    // variance every time, quirk Q2; PI2 / SPSA / warm-started CEM: the mean it has just written to prev_mean)
    const bool keep_init = LINGER && OPT != FOPT_RS && p.HU <= nthr;
    [[maybe_unused]] float m_keep = 0.0f, v_keep = 0.0f, s_keep = 0.0f;
    // ---- distribution init (cem.py:129-132 starts every control step from the ctor mean/var, quirk Q2)
    auto dist_init = [&](bool from_keep) {
        if (from_keep) {                     // resident pass: no global round trip
            if (tid < p.HU) {
                mean[tid] = m_keep;
                var[tid] = v_keep;
                sigma[tid] = (OPT == FOPT_CEM && p.warm_start) ? cem_sigma(m_keep, v_keep, lo, hi) : s_keep;
            }
        } else {
            for (int j = tid; j < p.HU; j += nthr) {
                const float m = p.prev_mean[a * p.HU + j];
                const float v = p.var0[a * p.HU + j];
                const float sg = (OPT == FOPT_CEM) ? cem_sigma(m, v, lo, hi) : ((OPT == FOPT_SPSA) ? 0.0f : sqrtf(v));
                mean[j] = m;
                var[j] = v;
                sigma[j] = sg;
                if (keep_init) { m_keep = m; v_keep = v; s_keep = sg; }
            }
        }
    };
    // (INJ == 2) the first two blocks of a thread's first trajectory are fetched while the PREVIOUS iteration selects and
    // refits (a resident pass: while the workgroup waits for its request): at the top of the rollout their loads would be
    // one exposed memory round trip per iteration
    typedef float pfvec4 __attribute__((ext_vector_type(4)));
    typedef const __attribute__((address_space(1))) pfvec4* pfvec4p;
    [[maybe_unused]] pfvec4 pf0 = {0.0f, 0.0f, 0.0f, 0.0f}, pf1 = {0.0f, 0.0f, 0.0f, 0.0f};
    [[maybe_unused]] auto prefetch_first = [&](const float* base, int it_n) {
        if constexpr (INJ == 2) {
            const int Q = (p.HU + 3) >> 2;
            if (tid < p.N) {                 // the lanes past the population roll nothing out
                const pfvec4p q = (pfvec4p)(reinterpret_cast<const float4*>(base) + noise_block_index(it_n, p.A, a, p.Nst, tid, Q));
                pf0 = q[0];
                if (OPT != FOPT_SPSA) pf1 = q[1];          // (Q == 1: past the row, never used -- noise_extent.hpp)
            }
        }
    };
    dist_init(false);
    __syncthreads();
    float s0 = red[60], s1 = red[61], s2 = red[62];
    if (p.iters > 0) prefetch_first(inj_s, 0);
    // ---- OptimizerBase.__call__ tail (optimizer_base.py:82-94), in two parts.
    // noise_term: the additive exploration term, from the bounds this thread holds in registers (no global reload behind
    // the carry stores).  It depends on the control step's key alone, not on the optimizer's result; evaluating it ahead of
    // the tail (in the iteration loop, while wave 0 waits for its SIMD mates) was built and put spill reloads into the
    // loop at this kernel's 128 registers: it stays in the tail (profiles/control_step_tail.md).
    auto noise_term = [&]() {
        FinalArgs fa;
        fa.A = p.A; fa.U = 1; fa.S = 3;
        fa.agent_offset = p.agent_offset;
        fa.fix_q1 = p.fix_q1; fa.fix_q7 = p.fix_q7;
        fa.add_noise = add_noise_s;
        fa.lo = p.lo; fa.hi = p.hi;
        fa.inj = p.inj_expl;
        fa.key = key_s;
        fa.key.q_per_agent = 1;
        return exploration_noise(fa, a, 0, lo, hi);                 // (resident form: every lane of wave 0 the same value)
    };
    // tail: apply the term, one model step, the record.  Launch-per-call form: thread 0 stores the packed record and
    // publishes with a release (publish_records_done).  Resident form: every lane of wave 0 computes the same five values
    // and lanes 0..15 store the agent's COMPLETION LINE, one word each, relaxed, with no fence in front -- the request
    // line's format mirrored: word 2f = (low half of float f) << 16 | tag, word 2f+1 = high half | tag, tag = the low 16 bits
    // of the sequence number; words 10..14 the tag alone, word 15 the whole sequence number.  The host accepts the line
    // when words 0..9 and 15 all name the call it waits for (completion_line.hpp), so neither the order in which the
    // words arrive nor how the fabric splits the store matters, and nothing has to be waited for in front of it.
    // CEM at the 512-thread register budget: the tail runs IN FRONT of the last iteration's closing statistics barrier, from
    // the row-0 mean thread 0 has just formed in a register (see the statistics below and the comment at the tail).  At 128
    // registers the same code put spill reloads into the selection (profiles/control_step_tail.md).
    constexpr bool EARLY_TAIL = BBMPC_FUSED_EARLY_TAIL && MAXT == 512 && OPT == FOPT_CEM;
    const bool tail_lanes = LINGER ? tid < 64 : tid == 0;
    auto tail = [&](float act_in) {
        BB_DBG(38);
        float s[3] = {s0, s1, s2};
        // EARLY_TAIL puts this model step inside the iteration loop, where the state is loop-invariant: left alone, the
        // compiler hoists sin(theta + pi) in front of the loop as +15 sin and forms acc = 3u - 15 sin here.  Equal for every
        // finite value, but a NaN state then leaves the step with its sign bit set where the other forms' -15 sin + 3u
        // leaves it clear.  The state is made opaque here so that the step is compiled in place, operation for operation
        // as written (models.hpp), and the record's bits are the same in every form, NaNs included.
        if constexpr (EARLY_TAIL) asm volatile("" : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]));
        float act[1];
        act[0] = add_noise_s ? exploration_apply(act_in, noise_term(), lo, hi) : act_in;
        BB_DBG(35);
        const float r = model.step(s, act);
        BB_DBG(36);
        if constexpr (LINGER) {
            const unsigned tag = done_value_s & 0xffffu;
            const float f = tid < 2 ? act[0] : (tid < 4 ? s[0] : (tid < 6 ? s[1] : (tid < 8 ? s[2] : r)));
            const unsigned bits = __float_as_uint(f);
            unsigned w = ((tid & 1) ? (bits & 0xffff0000u) : (bits << 16)) | tag;
            if (tid >= 10) w = tag;
            if (tid == 15) w = done_value_s;
            if (tid < 16) __hip_atomic_store(p.done_flag + a * 16 + tid, w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            BB_DBG(37);
        } else {
            float* rec = p.record + (size_t)a * 5;
            rec[0] = act[0];
            rec[1] = s[0];
            rec[2] = s[1];
            rec[3] = s[2];
            rec[4] = r;
            if (p.next_state) {
                p.next_state[a * 3 + 0] = s[0];
                p.next_state[a * 3 + 1] = s[1];
                p.next_state[a * 3 + 2] = s[2];
            }
            BB_DBG(37);
            // "records ready" for the all-gather that waits on another stream (comm.hpp): the last agent's workgroup
            // publishes the sequence number once every agent's record is in HBM.  No event, no extra packet on the
            // launch stream.
            publish_records_done(p.done_flag, p.done_count, done_value_s, gridDim.x);
        }
        BB_DBG(43);      // completion stored; slot 42: this pass's request accepted, 44: its first model step
    };
    for (;;) {      // one pass per control step; a single pass unless LINGER
        // (a resident pass arrives here with the distribution in LDS, the state in s0..s2 and its first draws on their way:
        // see the hand-off at the end of the loop)

        float action0 = (OPT == FOPT_RS) ? 0.0f : mean[0];          // iters == 0 -> untouched mean[:,0]

        BB_DBG(0);
#ifdef BBMPC_KERNEL_DBG
        if (p.dbg && tid == 0 && a == 0) dbg_lds[40] = (long long)clock64();
#endif
        for (int it = 0; it < p.iters; ++it) {
            BB_DBG(1 + it * 4);
            // ---- sample + rollout: one lane per trajectory, state in VGPRs
            // The 4 candidate actions of Philox block b+1 are generated while the recurrence steps through
            // block b: their instructions carry no dependence on the state, so they fill the latency
            // shadows of the sequential theta/thdot chain (all straight-line code inside a block).
            const float* inj = (INJ == 1) ? inj_s + ((size_t)it * p.A + a) * p.HU * p.Nst : nullptr;
            const int nblk = p.H >> 2, rem = p.H & 3;
            const uint32_t rstream = (OPT == FOPT_RS) ? 2u : 1u;
            // ILP independent trajectories per lane: with half as many waves each SIMD runs a single wave whose two
            // recurrences interleave in program order, instead of two waves fighting over issue slots.
            // quirk Q1's choice of the action-cost term is uniform for the launch: ONE branch here and a rollout body instantiated
            // for either value, instead of a second fma and a select in every model step (the op-for-op model resolves the
            // quirk inside its reward function: a single body)
            auto with_q1 = [&](auto&& body) {
                if constexpr (FASTM) {
                    if (p.fix_q1 != 0) { body(std::true_type{}); return; }
                }
                body(std::false_type{});
            };
            if constexpr (OPT == FOPT_SPSA) {
                // SPSA (spsa.py:61-107): theta +- c_k * delta with delta in {-1,+1}; both candidates of a particle are
                // rolled out by the same lane (two independent recurrences: four chains per SIMD at N = 500).  The
                // Rademacher draws stay in LDS (samp) for the gradient estimate.
                const float ck = p.spsa_ck[it];
                const int nb4 = (p.H + 3) >> 2;
                with_q1([&](auto Q1c) {
                constexpr bool Q1 = decltype(Q1c)::value;
                for (int n = tid; n < p.N; n += nthr) {
                    Roller<FASTM> rp, rm;
                    rp.init(p.fix_q1 != 0, s0, s1, s2);
                    rm.init(p.fix_q1 != 0, s0, s1, s2);
                    float tp = 0.0f, tm = 0.0f, pp = 0.0f, pm = 0.0f;
                    // (a GLOBAL pointer, said so: as a generic pointer -- inj_s may have come out of the mailbox -- its loads are
                    // flat loads, which count on the LDS counter as well: the mean[t] reads below then wait for the prefetch)
                    typedef float gvec4s __attribute__((ext_vector_type(4)));
                    typedef const __attribute__((address_space(1))) gvec4s* gvec4sp;
                    [[maybe_unused]] gvec4sp mine4 = nullptr;
                    [[maybe_unused]] gvec4s cur4 = {1.0f, 1.0f, 1.0f, 1.0f};
                    if constexpr (INJ == 2) {            // draws prefetched by k_noise_fill, one float4 per 4 steps
                        // (the row stride is prefetch_first's Q, from which pf0 came; the host requires U == 1 for this layout,
                        // Engine::optimize_fused, and then nb4 == Q blocks are walked)
                        mine4 = (gvec4sp)(reinterpret_cast<const float4*>(inj_s) + noise_block_index(it, p.A, a, p.Nst, n, (p.HU + 3) >> 2));
                        if (n == tid) cur4 = pf0;                    // fetched while the previous iteration refitted
                        else cur4 = mine4[0];
                    }
                    for (int b = 0; b < nb4; ++b) {
                        float d[4];
                        if constexpr (INJ == 2) {
                            const gvec4s nxt4 = mine4[b + 1];        // (the last one: past the row, never used -- noise_extent.hpp)
                            d[0] = cur4.x; d[1] = cur4.y; d[2] = cur4.z; d[3] = cur4.w;
                            cur4 = nxt4;
                        } else if (INJ == 1) {
#pragma unroll
                            for (int i = 0; i < 4; ++i) d[i] = (4 * b + i < p.H) ? inj[(size_t)(4 * b + i) * p.Nst + n] : 1.0f;
                        } else {
                            const U4 w = rng_block(key_s, 3u, (uint32_t)it, (uint32_t)n, (uint32_t)(p.agent_offset + a), (uint32_t)(4 * b));
                            d[0] = word_to_rademacher(w.x); d[1] = word_to_rademacher(w.y);
                            d[2] = word_to_rademacher(w.z); d[3] = word_to_rademacher(w.w);
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int t = 4 * b + i;
                            if (t < p.H) {
                                const float th = mean[t], stp = ck * d[i];
                                const float xp = th + stp, xm = th - stp;                      // spsa.py:76-77
                                const float xpf = clipf(xp, lo, hi), xmf = clipf(xm, lo, hi);  // :78-81
                                const float dp = xp - xpf, dm = xm - xmf;
                                pp = pp + dp * dp;
                                pm = pm + dm * dm;
                                samp[(size_t)t * p.Nst + n] = d[i];
                                rp.template step_acc_q1<Q1>(xpf);
                                rm.template step_acc_q1<Q1>(xmf);
                            }
                        }
                    }
                    tp = rp.total(); tm = rm.total();
                    if (tp != tp) tp = -1.0e6f;                                                // deterministic.py:75-77
                    if (tm != tm) tm = -1.0e6f;
                    const float np_ = sqrtf(pp), nm_ = sqrtf(pm);                              // tf.norm(...)**2  spsa.py:82-89
                    const float r_p = tp - np_ * np_, r_m = tm - nm_ * nm_;                    // :98-99
                    if (p.t_rewards) {
                        p.t_rewards[((size_t)it * p.A + a) * p.Nst + n] = r_p;
                        p.t_rewards2[((size_t)it * p.A + a) * p.Nst + n] = r_m;
                    }
                    rew[n] = r_p - r_m;
                }
                });
            } else if constexpr (INJ == 2) {
                // Draws prefetched by idle CUs (k_noise_fill): one float4 = one Philox block = 4 steps of this trajectory.
                // Loads run TWO blocks (8 steps, ~2 us) ahead of their use so that L2/HBM latency never reaches the
                // recurrence; the Philox rounds (a quarter of this kernel's VALU work) are gone from the critical path.
                const int Q = (p.HU + 3) >> 2;
                const float4* inj4 = reinterpret_cast<const float4*>(inj_s);
                // The rollout is bound by instruction issue, so what is uniform for the launch is decided ONCE
                // here and not once per model step: quirk Q1's choice of the action-cost term (Q1c) and the row stride of
                // samp[t][n] (NSTc: a compile-time stride turns the sample stores' addresses into immediate offsets of one
                // per-trajectory base; 0 = the run-time stride p.Nst).
                auto rollout = [&](auto Q1c, auto NSTc) {
                constexpr bool Q1 = decltype(Q1c)::value;
                constexpr int NSTC = decltype(NSTc)::value;
                const size_t nst = NSTC ? (size_t)NSTC : (size_t)p.Nst;
                for (int n = tid; n < p.N; n += nthr) {
                    Roller<FASTM> roll;
                    roll.init(p.fix_q1 != 0, s0, s1, s2);
                    float pen = 0.0f;
                    float* sp = samp + n;                          // compile-time stride: samp[4b + row][n] = sp[row * nst] for the block b it
                                                                   // stands at; run-time stride: the row of the next model step
                    // (a GLOBAL pointer, said so: inj_s may have come out of the mailbox, and as a generic pointer its loads are
                    // flat loads -- which count on the LDS counter too, so that every LDS wait of the loop below waited for the
                    // block it had just prefetched: one memory round trip per eight model steps)
                    typedef float gvec4 __attribute__((ext_vector_type(4)));
                    typedef const __attribute__((address_space(1))) gvec4* gvec4p;
                    // The pointer WALKS the row, and a load names its block by a constant distance from it (an immediate offset).
                    // It steps two blocks at the TOP of a trip (there the add's result can take the register of its operand;
                    // stepped at the foot, the add is scheduled in front of the trip's last load and costs a copy), so it
                    // stands at the trip's first block inside a trip and TWO BLOCKS BEHIND the block the code is at outside one:
                    // `ahead` below counts from the pointer.  No clamp at the row's end: the last trip's loads of blocks b + 2 /
                    // b + 3 may lie up to two float4 past the row -- in the next row or in the pad behind the chunk buffer
                    // (noise_extent.hpp) -- and are never used.
                    gvec4p mine = (gvec4p)((uintptr_t)(inj4 + noise_block_index(it, p.A, a, p.Nst, n, Q)) - 2 * sizeof(float4));
                    auto ld = [&](int ahead) { const gvec4 v = mine[ahead]; return make_float4(v.x, v.y, v.z, v.w); };
                    // sigma[4b .. 4b + 3] / mean[4b .. 4b + 3] (16-byte aligned, padded to a multiple of four) are read ONE block ahead
                    // of the model steps that use them: behind the previous block's recurrence, not in front of their own, where
                    // the LDS round trip stopped the chain at the top of every block.  Two bases that walk with the loop as the
                    // draws' pointer does (two blocks behind outside a trip), the block named by its constant distance from them.  No clamp: with H a multiple of four the last block
                    // reads one float4 past sigma[HUp] and mean[HUp], which the carve keeps inside this workgroup's LDS (see
                    // the invariant at the carve), and nobody uses it.
                    // (The bases are LDS addresses held in VGPRs, and the compiler is not told that they are uniform: knowing it,
                    // it walks them in SGPRs and pays a scalar add and a v_mov per block to hand each to the LDS instruction.)
                    struct SigMean { float4 sg, mn; };
                    typedef const __attribute__((address_space(3))) gvec4* lvec4p;
                    uint32_t sga = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)sigma - 2 * (uint32_t)sizeof(float4);
                    uint32_t mna = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)mean - 2 * (uint32_t)sizeof(float4);
                    asm volatile("" : "+v"(sga), "+v"(mna));
                    auto rd = [&](int ahead) {
                        SigMean r;
                        if (OPT == FOPT_RS) {
                            r.sg = r.mn = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        } else {
                            const gvec4 sg = ((lvec4p)(uintptr_t)sga)[ahead], mn = ((lvec4p)(uintptr_t)mna)[ahead];
                            r.sg = make_float4(sg.x, sg.y, sg.z, sg.w);
                            r.mn = make_float4(mn.x, mn.y, mn.z, mn.w);
                        }
                        return r;
                    };
                    auto action = [&](float xi, float sg, float mn) { return (OPT == FOPT_RS) ? xi * (hi - lo) + lo : xi * sg + mn; };
                    // one model step on action x, row `row` (a constant at every call) of the block sp stands at
                    auto step1 = [&](int row, float x) {
                        if (OPT == FOPT_PI2) {
                            const float xf = clipf(x, lo, hi);
                            const float d = x - xf;
                            pen = pen + d * d;
                            x = xf;
                        }
                        if constexpr (NSTC != 0) {
                            sp[(size_t)row * nst] = x;           // an immediate offset from the block's base
                        } else {
                            *sp = x;                             // run-time stride: the pointer walks the rows
                            sp += nst;
                        }
                        roll.template step_acc_q1<Q1>(x);
                    };
                    // Block b: its four actions are formed from its draws z and from m = sigma / mean of block b BEFORE its model
                    // steps (inside the steps they would sit between the sine and the angle update of the recurrence).  That is
                    // the last use of both, so the loads of block b + 2's draws and of block b + 1's sigma / mean are issued
                    // right there INTO THE SAME REGISTERS and run beside this block's recurrence: no copy at a loop's foot, and
                    // neither the memory nor the LDS round trip ever stands in front of a model step.
                    SigMean m = rd(2);
                    auto block4 = [&](float4& z, int ahead, int row0, bool more) {      // ahead: blocks from where the bases stand to this one
                        float x[4] = {action(z.x, m.sg.x, m.mn.x), action(z.y, m.sg.y, m.mn.y), action(z.z, m.sg.z, m.mn.z), action(z.w, m.sg.w, m.mn.w)};
#if BBMPC_FUSED_ACTIONS_AHEAD
#pragma unroll
                        for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(x[i]));
#endif
                        if (more) z = ld(ahead + 2);             // draws: two blocks (8 steps, ~2 us) ahead of their use
                        m = rd(ahead + 1);                       // (also what the remainder steps behind the last block use)
#pragma unroll
                        for (int i = 0; i < 4; ++i) step1(row0 + i, x[i]);
                    };
                    float4 c0, c1;
                    if (n == tid) { c0 = make_float4(pf0.x, pf0.y, pf0.z, pf0.w); c1 = make_float4(pf1.x, pf1.y, pf1.z, pf1.w); }   // fetched an iteration ago
                    else { c0 = ld(2); c1 = ld(3); }
#ifdef BBMPC_KERNEL_DBG
                    if (it == 0 && n == tid) { asm volatile("" :: "v"(c0.x)); BB_DBG(44); }     // the first draws are there
#endif
                    // (Waves that share a SIMD run the same instruction stream and the arbiter favours the older one; pacing
                    // them against each other through LDS progress words or s_setprio was measured slower both times and is
                    // gone: profiles/rollout_loop_issue_slots.md 5.  BBMPC_BALANCE is still accepted and does nothing.)
                    for (int trips = nblk >> 1; trips > 0; --trips) {      // two blocks a trip; every base steps once
                        mine += 2;
                        sga += 2 * (uint32_t)sizeof(float4);
                        mna += 2 * (uint32_t)sizeof(float4);
                        asm volatile("" : "+v"(mine), "+v"(sga), "+v"(mna));      // three adds, not one shared scalar offset and an add per base per trip to apply it
                        block4(c0, 0, 0, true);
                        block4(c1, 1, 4, true);
                        if constexpr (NSTC != 0) sp += 8 * nst;
                    }
                    if (nblk & 1) { block4(c0, 2, 0, false); c0 = c1; if constexpr (NSTC != 0) sp += 4 * nst; }
                    if (rem > 0) step1(0, action(c0.x, m.sg.x, m.mn.x));
                    if (rem > 1) step1(1, action(c0.y, m.sg.y, m.mn.y));
                    if (rem > 2) step1(2, action(c0.z, m.sg.z, m.mn.z));
                    float tot = roll.total();
                    if (tot != tot) tot = -1.0e6f;                                   // deterministic.py:75-77
                    if (OPT == FOPT_PI2) {
                        const float nr = sqrtf(pen);
                        tot = tot - nr * nr;
                    }
                    rew[n] = tot;
                }
                };
                // (SAMPLES_LDS, Nst = 512 -- populations of 449 .. 512: the whole array lies within a ds_write's 64 KB of
                // immediate offset up to H = 31, and the compiler falls back to address arithmetic by itself beyond)
                auto rollout_q1 = [&](auto NSTc) { with_q1([&](auto Q1c) { rollout(Q1c, NSTc); }); };
                bool rolled = false;
                if constexpr (SAMPLES_LDS) {
                    if (p.Nst == 512) { rollout_q1(std::integral_constant<int, 512>{}); rolled = true; }
                }
                if (!rolled) rollout_q1(std::integral_constant<int, 0>{});
            } else
            with_q1([&](auto Q1c) {
            constexpr bool Q1 = decltype(Q1c)::value;
            for (int n0 = tid; n0 < p.N; n0 += ILP * nthr) {
                int nn[ILP];
                bool live[ILP];
                Roller<FASTM> roll[ILP];
                float pen[ILP], xn[ILP][4];
#pragma unroll
                for (int q = 0; q < ILP; ++q) {
                    live[q] = n0 + q * nthr < p.N;
                    nn[q] = live[q] ? n0 + q * nthr : n0;          // idle slots shadow particle n0 (never stored)
                    roll[q].init(p.fix_q1 != 0, s0, s1, s2);
                    pen[q] = 0.0f;
                }
                auto gen = [&](int q, int b) {
                    const int n = nn[q];
                    float xi[4];
                    if (INJ) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) xi[i] = (4 * b + i < p.H) ? inj[(size_t)(4 * b + i) * p.Nst + n] : 0.0f;
                    } else {
                        const U4 w = rng_block(key_s, rstream, (uint32_t)it, (uint32_t)n, (uint32_t)(p.agent_offset + a),
                                               (uint32_t)(4 * b));
                        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            xi[i] = (OPT == FOPT_RS) ? word_to_uniform(ww[i]) : word_to_trunc_normal(ww[i]);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int t = min(4 * b + i, p.H - 1);
                        if (OPT == FOPT_RS) xn[q][i] = xi[i] * (hi - lo) + lo;      // random_search.py:40-41
                        else xn[q][i] = xi[i] * sigma[t] + mean[t];                 // cem.py:90-94 / pi2.py:65-69
                    }
                };
                auto consume = [&](int q, int t, float x) {
                    if (OPT == FOPT_PI2) {                                           // pi2.py:70-75
                        const float xf = clipf(x, lo, hi);
                        const float d = x - xf;
                        pen[q] = pen[q] + d * d;
                        x = xf;
                    }
                    if (live[q]) samp[(size_t)t * p.Nst + nn[q]] = x;
                    roll[q].template step_acc_q1<Q1>(x);     // (the H-step sum is the roller's: the same form as the prefetched-draws path above, bit for bit)
                };
#pragma unroll
                for (int q = 0; q < ILP; ++q) gen(q, 0);
                for (int b = 0; b < nblk; ++b) {
                    float xc[ILP][4];
#pragma unroll
                    for (int q = 0; q < ILP; ++q) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) xc[q][i] = xn[q][i];
                        gen(q, b + 1);       // one block ahead (the block past the end is generated and dropped)
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int q = 0; q < ILP; ++q) consume(q, 4 * b + i, xc[q][i]);
                }
                for (int i = 0; i < rem; ++i)
#pragma unroll
                    for (int q = 0; q < ILP; ++q) consume(q, 4 * nblk + i, xn[q][i]);
#pragma unroll
                for (int q = 0; q < ILP; ++q) {
                    float tot = roll[q].total();
                    if (tot != tot) tot = -1.0e6f;                                   // deterministic.py:75-77
                    if (OPT == FOPT_PI2) {
                        const float nr = sqrtf(pen[q]);
                        tot = tot - nr * nr;
                    }
                    if (live[q]) rew[nn[q]] = tot;
                }
            }
            });
#ifdef BBMPC_KERNEL_DBG
            if (p.dbg && a == 0 && it == 0 && (tid & 63) == 0) dbg_lds[24 + (tid >> 6) % 8] = (long long)wall_clock64();
#endif
            // the selection's first part reads only the rewards this thread has just written: in front of the barrier the
            // rollout needs anyway instead of behind it with a barrier of its own (topk.hpp)
            if (it + 1 < p.iters) prefetch_first(inj_s, it + 1);
            if constexpr (WAVE_SEL) block_topk_prepass<true, true>(rew, p.N, p.k, hist, tid, nthr, slot_min, slot_bound);
            else if (OPT == FOPT_CEM) block_topk_prepass(rew, p.N, p.k, hist, tid, nthr);
            BB_DBG(2 + it * 4);
            __syncthreads();
            BB_DBG(3 + it * 4);
            if (p.t_rewards) {
                if (OPT != FOPT_SPSA)
                    for (int n = tid; n < p.N; n += nthr) p.t_rewards[((size_t)it * p.A + a) * p.Nst + n] = rew[n];
                for (int i = tid; i < p.HU * p.Nst; i += nthr) {
                    const int j = i / p.Nst, n = i % p.Nst;
                    if (n < p.N) p.t_samples[(((size_t)it * p.A + a) * p.HU + j) * p.Nst + n] = samp[(size_t)j * p.Nst + n];
                }
            }

            // ---- refit
            if (OPT == FOPT_CEM) {
                // exact sorted top-k (tf.nn.top_k, cem.py:97-99): LDS radix select, see topk.hpp
                // The refit needs the elite SET only, so the winners are listed in ascending index order (no ranking);
                // the sorted list tf.nn.top_k returns is produced only for the parity trace.  The statistics below always
                // run over the index-ordered list, so results do not depend on tracing.
                TopkSel sel;
                [[maybe_unused]] int route = TOPK_ROUTE_OLD;
                if constexpr (WAVE_SEL) {
                    // the common case only: one element per thread, k <= 64, tracing off; every other case, and every
                    // selection the route declines, runs today's code (uniform for the workgroup either way)
                    if (p.wave_select && p.t_elites == nullptr && p.N <= nthr && p.k <= 64)
                        route = block_topk_wave_select(rew, p.N, p.k, eidx, hist, slot_min, slot_bound, tid, nthr, sel);
                    else
                        sel = block_topk_select(rew, p.N, p.k, hist, tid, nthr, true, slot_min, slot_bound);
                } else {
                    sel = block_topk_select(rew, p.N, p.k, hist, tid, nthr, true);
                }
                // (null unless traced; bit 8: the all-wave route listed the winners)
                if (p.t_passes && tid == 0) p.t_passes[(size_t)it * p.A + a] = sel.passes | (route != TOPK_ROUTE_OLD ? 0x100 : 0);
                if (route == TOPK_ROUTE_OLD) {
                    if (p.t_elites) {
                        block_topk_finish_sorted(rew, p.N, p.k, eidx, hist, ekeys, sel, tid, nthr);
                        for (int e = tid; e < p.k; e += nthr) p.t_elites[((size_t)it * p.A + a) * p.k + e] = eidx[e];
                        __syncthreads();
                    }
                    block_topk_finish_indexed(rew, p.N, p.k, eidx, hist, sel, tid, nthr);
                }
                BB_DBG(4 + it * 4);
#ifdef BBMPC_KERNEL_DBG
                if (p.dbg && tid == 0 && a == 0 && it == 1) for (int i = 0; i < 12; ++i) p.dbg[48 + i] = g_topk_dbg[i];
#endif
                // elite statistics (cem.py:112-125): one 16-lane DPP row per (h,u) element -- 4 elements per wave,
                // every element of the horizon at once for H*U <= 4*waves; mean and biased variance two-pass,
                // as the reference computes them.
                const float kf = (float)p.k;
                const int sub = tid & 15;
                // up to 64 elites: a lane's (<= 4) elite indices and sample values stay in registers -- every LDS read of
                // a phase is issued before the first use (a dependent eidx -> row read per element costs two LDS
                // latencies each, 16 in a row for k = 50)
                constexpr int EC = 4;
                const bool small_k = p.k <= 16 * EC;
                int ei[EC];
#pragma unroll
                for (int i = 0; i < EC; ++i) ei[i] = (small_k && sub + 16 * i < p.k) ? eidx[sub + 16 * i] : -1;
                [[maybe_unused]] float mean_row0 = 0.0f;      // EARLY_TAIL: thread 0's copy of the mean[0] it stores below
                for (int j = tid >> 4; j < ((p.HU + 3) & ~3); j += nthr >> 4) {       // all 16 lanes of a row share j
                    const bool live = j < p.HU;
                    const float* row = samp + (size_t)(live ? j : 0) * p.Nst;
                    float sum = 0.0f, vs = 0.0f, em;
                    if (small_k) {
                        float x[EC];
#pragma unroll
                        for (int i = 0; i < EC; ++i) x[i] = row[ei[i] >= 0 ? ei[i] : 0];
#pragma unroll
                        for (int i = 0; i < EC; ++i) if (ei[i] >= 0) sum += x[i];
                        sum = row16_sum(sum);
                        em = sum / kf;                                               // cem.py:112
#pragma unroll
                        for (int i = 0; i < EC; ++i)
                            if (ei[i] >= 0) {
                                const float d = x[i] - em;
                                vs += d * d;
                            }
                    } else {
                        for (int e = sub; e < p.k; e += 16) sum += row[eidx[e]];
                        sum = row16_sum(sum);
                        em = sum / kf;
                        for (int e = sub; e < p.k; e += 16) {
                            const float d = row[eidx[e]] - em;
                            vs += d * d;
                        }
                    }
                    vs = row16_sum(vs);
                    if (live && sub == 0) {
                        const float ev = vs / kf;                                    // cem.py:113-119
                        const float one_m = 1.0f - p.alpha;
                        const float m = p.alpha * mean[j] + one_m * em;              // cem.py:121-122
                        const float v = p.alpha * var[j] + one_m * ev;               // cem.py:123-125
                        mean[j] = m;
                        var[j] = v;
                        sigma[j] = cem_sigma(m, v, lo, hi);
                        if constexpr (EARLY_TAIL) { if (j == 0) mean_row0 = m; }     // (row 0 is thread 0's, in its first trip)
                    }
                }
                if (it == 0) BB_DBG(33);
                if constexpr (EARLY_TAIL) {
                    // The last iteration: the caller needs mean[0] only, and thread 0 holds the very float it has just stored
                    // there.  Wave 0 runs the tail from it and stores the completion line / the record without waiting for the
                    // other rows' statistics; it then joins the barrier below like every wave (no barrier is skipped, so the
                    // order of every LDS access on either side of it is what it was).
                    if (it + 1 == p.iters && tail_lanes) {
                        tail(__int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mean_row0))));   // (wave 0's first lane is thread 0)
                    }
                }
                __syncthreads();
                action0 = mean[0];                                                   // cem.py:135
            } else if (OPT == FOPT_PI2) {
                // pi2.py:78-87.  Cross-wave reductions use their own LDS slots (no second barrier to recycle them) and the
                // per-wave slots are combined by every wave with one LDS round trip + a DPP reduction.
                float lmin = INFINITY;
                for (int n = tid; n < p.N; n += nthr) {
                    const float c = -rew[n];                                         // pi2.py:78
                    rew[n] = c;
                    lmin = fminf(lmin, c);
                }
                lmin = wave_min(lmin);
                if ((tid & 63) == 0) red[tid >> 6] = lmin;
                __syncthreads();
                float beta = ((tid & 63) < nw) ? red[tid & 63] : INFINITY;
                beta = wave_min(beta);                                               // pi2.py:81
                float lsum = 0.0f;
                for (int n = tid; n < p.N; n += nthr) {
                    const float pr = expf((-p.inv_lamda) * (rew[n] - beta));         // pi2.py:82
                    rew[n] = pr;
                    lsum += pr;
                }
                lsum = wave_sum(lsum);
                if ((tid & 63) == 0) red[32 + (tid >> 6)] = lsum;
                __syncthreads();
                float eta = ((tid & 63) < nw) ? red[32 + (tid & 63)] : 0.0f;
                eta = wave_sum(eta);                                                 // pi2.py:83
                const float inv_eta = 1.0f / eta;
                // new_mean[j] = sum_n x[j][n] * omega[n],  omega = inv_eta * prob   (pi2.py:85-87): one wave per j
                for (int j = tid >> 6; j < p.HU; j += nw) {
                    const float* row = samp + (size_t)j * p.Nst;
                    float acc = 0.0f;
                    for (int n = tid & 63; n < p.N; n += 64) acc += row[n] * (inv_eta * rew[n]);
                    acc = wave_sum(acc);
                    if ((tid & 63) == 0) mean[j] = acc;
                }
                __syncthreads();
                action0 = mean[0];                                                   // pi2.py:94
            } else if (OPT == FOPT_SPSA) {
                // ghat[j] = mean_n (r+ - r-)[n] / (2 c_k delta[j][n]);  theta = clip(theta + a_k ghat)   (spsa.py:101-107)
                const float two_ck = 2.0f * p.spsa_ck[it], ak = p.spsa_ak[it];
                for (int j = tid >> 6; j < p.HU; j += nw) {
                    const float* row = samp + (size_t)j * p.Nst;
                    float acc = 0.0f;
                    for (int n = tid & 63; n < p.N; n += 64) acc += rew[n] / (two_ck * row[n]);
                    acc = wave_sum(acc);
                    if ((tid & 63) == 0) mean[j] = clipf(mean[j] + ak * (acc / (float)p.N), lo, hi);
                }
                __syncthreads();
                action0 = mean[0];                                                   // spsa.py:117
            } else {  // RandomSearch: argmax, first maximum (random_search.py:43-47)
                float bv = -INFINITY;
                int bi = 0x7fffffff;
                for (int n = tid; n < p.N; n += nthr) {
                    const float v = rew[n];
                    if (v > bv || (v == bv && n < bi)) { bv = v; bi = n; }
                }
                wave_argmax(bv, bi);
                int* redi = (int*)(red + 32);
                if ((tid & 63) == 0) { red[tid >> 6] = bv; redi[tid >> 6] = bi; }
                __syncthreads();
                bv = ((tid & 63) < nw) ? red[tid & 63] : -INFINITY;
                bi = ((tid & 63) < nw) ? redi[tid & 63] : 0x7fffffff;
                wave_argmax(bv, bi);
                if (bi == 0x7fffffff) bi = 0;
                action0 = samp[bi];                                                  // sample[best][t=0]
                if (p.t_elites && tid == 0) p.t_elites[a] = bi;
                __syncthreads();
            }
            if (p.t_mean && OPT != FOPT_RS)
                for (int j = tid; j < p.HU; j += nthr) {
                    p.t_mean[((size_t)it * p.A + a) * p.HU + j] = mean[j];
                    p.t_var[((size_t)it * p.A + a) * p.HU + j] = var[j];
                }
        }

        BB_DBG(1 + p.iters * 4);
#ifdef BBMPC_KERNEL_DBG
        if (p.dbg && tid == 0 && a == 0) dbg_lds[41] = (long long)clock64();
#endif
        // ---- OptimizerBase.__call__ tail (optimizer_base.py:82-94).  (Running it from thread 0's own row-0 mean in front of
        // CEM's last statistics barrier was built too: inlined into the iteration loop it put spill reloads into the
        // selection, profiles/control_step_tail.md.)
        // The 512-thread CEM form (EARLY_TAIL) has run it already, in front of the last statistics barrier, from thread 0's
        // register copy of mean[0] -- the float action0 holds here; only a control step without iterations comes by.
        if (tail_lanes && !(EARLY_TAIL && p.iters > 0)) tail(action0);
        // ---- state carried to the next control step, BEHIND the publish: the caller waits for the record, not for these.
        // Invariant this rests on: nothing reads mean_out / var_out / prev_mean between the completion and the end of
        // the kernel -- with EARLY_TAIL the completion precedes the last statistics barrier as well, i.e. the other rows'
        // mean[] / var[] / sigma[] are still being written in LDS when the caller has its record; nothing outside the
        // workgroup reads LDS, and the global copies are stored below as before.  The host's readers (bbmpc_get_state, the traces, every entry point but bbmpc_optimize,
        // bbmpc_optimize_gather and bbmpc_gather_wait) settle the handle first -- Engine::settle ends a resident kernel and
        // joins the stream -- and the next control step is either a launch on the same stream or a resident pass, which
        // starts from the registers kept here (m_keep), or from the copies this very thread stores below.
        if (OPT != FOPT_RS) {
            for (int j = tid; j < p.HU; j += nthr) {
                p.mean_out[a * p.HU + j] = mean[j];
                p.var_out[a * p.HU + j] = var[j];
                if (OPT == FOPT_PI2 || OPT == FOPT_SPSA) {                           // shift-left warm start pi2.py:92-93 / spsa.py:114-115
                    const int js = (j + 1 < p.HU) ? j + 1 : p.HU - 1;
                    const float pm = mean[js];
                    p.prev_mean[a * p.HU + j] = pm;
                    if (keep_init) m_keep = pm;
                } else if (p.warm_start) {
                    const float pm = mean[j];
                    p.prev_mean[a * p.HU + j] = pm;
                    if (keep_init) m_keep = pm;
                }
            }
        }
        BB_DBG(34);
#ifdef BBMPC_KERNEL_DBG
        if (p.dbg && a == 0 && tid == 0) for (int i = 0; i < 48; ++i) p.dbg[i] = dbg_lds[i];
#endif
        if constexpr (!LINGER) {
            break;
        } else {
            // ---- stay resident: wave 0 polls the request line over PCIe (one 64-byte read per poll).  Words 0..12 of a
            // request carry 16 bits of payload each plus the low 16 bits of the request's sequence number, word 15 the
            // whole number (Engine::resident_step): a line is accepted when ALL fourteen words name the request this
            // workgroup waits for, so neither the order of the host's stores nor how the fabric splits the read matters.
            // A request carrying the NEXT sequence number starts another pass without a launch (measured: 2.1 us
            // host-to-host for a resident kernel's mailbox round trip against 6.8 us for launch + completion,
            // tools/microbench/launch_latency.hip); the stop word in word 15, or linger_ticks without a request, ends the
            // kernel, which says so in `gone` first and never looks at the line again, so the host knows whether to launch.
            // Everything the next pass needs that does not depend on the request is staged BEFORE the poll: its starting
            // distribution goes to LDS (from the kept registers, or -- RandomSearch, H*U > threads -- from the global copies
            // this thread has just written itself), and every thread fetches its first draws from where the next request
            // will most likely point.  Behind the request there is one barrier.  (Wave 0 fetches its draws in front of the
            // poll like everybody else: its first read of the request line waits for them, a device-memory round trip at a
            // moment when the host has not even seen this pass's completion line.)
            // The answer goes back the same way (the kernel's tail above): a self-validating 64-byte completion line per
            // agent that carries the record itself, stored by relaxed stores with nothing waited for in front; the state
            // carried to the next step (mean_out / var_out / prev_mean) is stored behind it, off the caller's critical path.
            // A workgroup that leaves has stored the line of every step it served before it says so in `gone` (a release).
            // The request's 16 words are handed to the other waves in red[16..31], which nothing else ever writes.  They
            // used to go through ekeys[]: with num_elite = 0 (PI2, SPSA, RandomSearch) or < 8 that piece of the carve is
            // shorter than 16 words and the words lay on samples[0][0..15], which wave 0 stores in its first model step of
            // the next pass -- with no barrier between that store and the other waves' reads below.  A late wave then
            // decoded part of its state from sample values: config 3 (PI2, 8 agents x 16 waves) gave other results in
            // a few of every ten 200-step runs, depending on nothing but timing.
            unsigned* mb = (unsigned*)(red + 16);
            // (EARLY_TAIL: wave 0 left the last iteration's statistics early for the tail, but it took part in that
            // iteration's closing barrier and takes part in this one like every wave, so its dist_init stores to mean[] /
            // var[] / sigma[] below are still ordered behind every wave's last reads of them: the carry loop above.)
            __syncthreads();                                       // mean[] / ekeys / red have been read for the last time
            dist_init(keep_init);
            [[maybe_unused]] const float* inj_pred = nullptr;
            if constexpr (INJ == 2) {
                if (p.pf_step_floats)
                    for (int b = 0; b < 2; ++b)
                        if (inj_s >= p.pf_buf[b] && inj_s + 2 * p.pf_step_floats <= p.pf_buf[b] + p.pf_chunk_floats) inj_pred = inj_s + p.pf_step_floats;
                if (inj_pred && p.iters > 0) prefetch_first(inj_pred, 0);
            }
            if (tid < 64) {
                const long long t0 = (long long)wall_clock64();
                const unsigned want = done_value_s + 1u;
                unsigned w = 0u;
                bool quit = false;
                for (;;) {
                    w = (tid < 16) ? __hip_atomic_load(p.mbox + a * 16 + tid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0u;
                    const bool mine = tid < 13 ? (w & 0xffffu) == (want & 0xffffu) : (tid == 15 ? w == want : true);
                    const unsigned w15 = __builtin_amdgcn_readlane(w, 15);
                    if (__builtin_amdgcn_ballot_w64(mine) == ~0ull) break;
                    if (w15 == 0xffffffffu || (long long)wall_clock64() - t0 > (long long)p.linger_ticks || a == p.test_quit_agent || (p.test_quit_agent >= 999 && a >= p.test_quit_agent - 999)) { quit = true; break; }
                }
                if (tid < 16) mb[tid] = (quit && tid == 15) ? 0xffffffffu : w;
                BB_DBG(42);
            }
            __syncthreads();
            if (mb[15] == 0xffffffffu) {
                if (tid == 0) __hip_atomic_store(p.gone + a * 16, done_value_s, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                return;
            }
            done_value_s = mb[15];
            key_s.step = (mb[0] >> 16) | (mb[1] & 0xffff0000u);
            add_noise_s = (int)(mb[2] >> 16);
            inj_s = reinterpret_cast<const float*>(((unsigned long long)(mb[3] >> 16)) | ((unsigned long long)(mb[4] >> 16) << 16) |
                                                   ((unsigned long long)(mb[5] >> 16) << 32) | ((unsigned long long)(mb[6] >> 16) << 48));
            // (every thread decodes the state itself; red[16..31] is not written again before the next pass's poll)
            s0 = __uint_as_float((mb[7] >> 16) | (mb[8] & 0xffff0000u));
            s1 = __uint_as_float((mb[9] >> 16) | (mb[10] & 0xffff0000u));
            s2 = __uint_as_float((mb[11] >> 16) | (mb[12] & 0xffff0000u));
            if (p.iters > 0 && inj_s != inj_pred) prefetch_first(inj_s, 0);      // nothing was predicted (the chunk's last step), or -- not
                                                                                 // reachable through the host's entry points today -- another pointer
        }
    }
}

}  // namespace bbmpc
