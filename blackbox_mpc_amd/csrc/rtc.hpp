// User-supplied reward / dynamics functions as DEVICE code compiled at run time (hiprtc).
//
// The reference accepts any callable as `reward_function` / `dynamics_function`
// (trajectory_evaluators/deterministic.py:13-18, called at :65-66 and :99-100; plugin contracts in SURVEY.md 1-L1):
//     reward  r(current_state[B,S], actions[B,U], next_state[B,S]) -> [B]
//     dynamics f(x[B,S+U], train) -> delta[B,S]           (true model: next = delta + state, transforms.py:34)
// Python callables cannot run inside a kernel, so the counterpart here is a HIP source string that defines
//     __device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U);
//     __device__ void  bbmpc_user_dynamics(const float* x /*[S+U]*/, float* delta /*[S]*/, int S, int U);
// per row.  bbmpc_set_reward_source / bbmpc_set_dynamics_source compile it together with the two row kernels below and
// the engine calls them once per planning step from its step-wise evaluator (kernels_user.hpp).  libhiprtc is bound at
// run time, next to the HIP runtime the process already uses; compiling needs no GPU.
//
// Runtime parameters (bbmpc_set_*_source_params): a source declared with P > 0 parameters defines instead
//     __device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
//                                               const float* params, int t);
//     __device__ void  bbmpc_user_dynamics_params(const float* x, float* delta, int S, int U, const float* params, int t);
// where `params` is the P-float row of the agent that owns the row (read only) and t the planning step (0 on one-step
// calls).  The programs are then compiled with BBMPC_REW_NPARAMS / BBMPC_DYN_NPARAMS = P, on which the kernel texts below
// select the parameterised call and the extra kernel arguments with the preprocessor (k_user_calls); without the define a
// kernel is exactly the classic one.  This header is the hiprtc side only; bbmpc_user.hip, the one unit that includes it,
// holds the Engine members that compile, load and launch the programs, and their C ABI entry points.
#pragma once
#include <dlfcn.h>
#include "../../include/bbmpc.h"   // bbmpc_rows_callback
#include <hip/hip_runtime.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace bbmpc {

struct Hiprtc {
    typedef void* Program;
    int (*CreateProgram)(Program*, const char*, const char*, int, const char**, const char**) = nullptr;
    int (*CompileProgram)(Program, int, const char**) = nullptr;
    int (*GetProgramLogSize)(Program, size_t*) = nullptr;
    int (*GetProgramLog)(Program, char*) = nullptr;
    int (*GetCodeSize)(Program, size_t*) = nullptr;
    int (*GetCode)(Program, char*) = nullptr;
    int (*DestroyProgram)(Program*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;

    static const Hiprtc& get() {
        static const Hiprtc api = load();
        return api;
    }

private:
    static Hiprtc load() {
        void* lib = dlopen("libhiprtc.so", RTLD_NOW | RTLD_NOLOAD);
        if (!lib) {
            // the copy that ships with the HIP runtime this process runs on (PyTorch bundles its own pair)
            Dl_info info;
            if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &info) && info.dli_fname) {
                std::string p(info.dli_fname);
                const size_t slash = p.rfind('/');
                if (slash != std::string::npos) lib = dlopen((p.substr(0, slash + 1) + "libhiprtc.so").c_str(), RTLD_NOW | RTLD_GLOBAL);
            }
        }
        const char* names[] = {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
        for (int i = 0; !lib && i < 3; ++i) lib = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
        if (!lib) throw std::runtime_error("libhiprtc.so not found (needed to compile user reward / dynamics device functions)");
        Hiprtc a;
        auto sym = [&](const char* s) {
            void* p = dlsym(lib, s);
            if (!p) throw std::runtime_error(std::string("libhiprtc: missing symbol ") + s);
            return p;
        };
        a.CreateProgram = reinterpret_cast<decltype(a.CreateProgram)>(sym("hiprtcCreateProgram"));
        a.CompileProgram = reinterpret_cast<decltype(a.CompileProgram)>(sym("hiprtcCompileProgram"));
        a.GetProgramLogSize = reinterpret_cast<decltype(a.GetProgramLogSize)>(sym("hiprtcGetProgramLogSize"));
        a.GetProgramLog = reinterpret_cast<decltype(a.GetProgramLog)>(sym("hiprtcGetProgramLog"));
        a.GetCodeSize = reinterpret_cast<decltype(a.GetCodeSize)>(sym("hiprtcGetCodeSize"));
        a.GetCode = reinterpret_cast<decltype(a.GetCode)>(sym("hiprtcGetCode"));
        a.DestroyProgram = reinterpret_cast<decltype(a.DestroyProgram)>(sym("hiprtcDestroyProgram"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("hiprtcGetErrorString"));
        return a;
    }
};

constexpr int USER_KIND_REWARD = 1, USER_KIND_DYNAMICS = 2;
// target transforms (SystemDynamicsHandler's transform_targets_func / inverse_transform_targets_func, reference
// dynamics_handlers/system_dynamics_handler.py:15-17, 128-161, 314):
//     __device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S);
//     __device__ void bbmpc_user_transform_targets(const float* cur, const float* next, float* target, int S);
constexpr int USER_KIND_INVERSE_TRANSFORM = 3, USER_KIND_TRANSFORM = 4;

// The two calls of a user function, for every program below and kernels_mlp_xform.hpp: the classic entry point, or with
// BBMPC_*_NPARAMS the parameterised one on row `agent` of `params` [A][P] (an argument only the parameterised kernel has).
static const char* const k_user_calls = R"RTC(
#ifdef BBMPC_REW_NPARAMS
#define BBMPC_CALL_REWARD(c, a, n, params, agent, t) bbmpc_user_reward_params(c, a, n, BBMPC_S, BBMPC_U, (params) + (size_t)(agent) * BBMPC_REW_NPARAMS, t)
#else
#define BBMPC_CALL_REWARD(c, a, n, params, agent, t) bbmpc_user_reward(c, a, n, BBMPC_S, BBMPC_U)
#endif
#ifdef BBMPC_DYN_NPARAMS
#define BBMPC_CALL_DYNAMICS(x, d, params, agent, t) bbmpc_user_dynamics_params(x, d, BBMPC_S, BBMPC_U, (params) + (size_t)(agent) * BBMPC_DYN_NPARAMS, t)
#else
#define BBMPC_CALL_DYNAMICS(x, d, params, agent, t) bbmpc_user_dynamics(x, d, BBMPC_S, BBMPC_U)
#endif
)RTC";

// The row kernels the engine launches around the user's function.  BBMPC_S / BBMPC_U are compile-time so the per-row
// arrays live in registers; rows are [batch, S] / [batch, astride] row-major.  A dynamics program with an inverse target
// transform (BBMPC_XFORM) applies it in place of next = delta + state.  A parameterised reward / dynamics: the row kernels
// take (params [A][P], rows_per_agent, t) -- row b belongs to agent b / rows_per_agent -- and the traj scorer takes params
// and reads the row of agent blockIdx.y.
static const char* const k_reward_rows_text = R"RTC(
extern "C" __global__ void bbmpc_user_reward_rows(const float* __restrict__ cur, const float* __restrict__ nxt,
                                                  const float* __restrict__ act, int astride, int batch,
                                                  float* __restrict__ total, int accumulate
#ifdef BBMPC_REW_NPARAMS
                                                  , const float* __restrict__ params, int rows_per_agent, int t
#endif
                                                  ) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float c[BBMPC_S], n[BBMPC_S], a[BBMPC_U];
    for (int i = 0; i < BBMPC_S; ++i) { c[i] = cur[(size_t)b * BBMPC_S + i]; n[i] = nxt[(size_t)b * BBMPC_S + i]; }
    for (int i = 0; i < BBMPC_U; ++i) a[i] = act[(size_t)b * astride + i];
    // reward_function(current_state, actions, next_state): the argument order of the CALL (deterministic.py:65-66)
    const float r = BBMPC_CALL_REWARD(c, a, n, params, b / rows_per_agent, t);
    total[b] = accumulate ? total[b] + r : r;
}

// The learned MLP's rollouts run on the matrix cores (kernels_mlp.hpp) and leave the state after every step in
// traj [H][A][Nst][S]; this scores the whole trajectory of one candidate per lane: sum_t r(s_t, a_t, s_t+1), NaN -> -1e6
// (deterministic.py:62-77).  `rewards` holds -(penalty) from the rollout kernel (0 without one): R - penalty.
extern "C" __global__ void bbmpc_user_reward_traj(int n_pop, int A, int H, int Nst, int from_ref,
                                                  const float* __restrict__ state, const float* __restrict__ traj,
                                                  const float* __restrict__ seq, const float* __restrict__ cand,
                                                  float* __restrict__ rewards
#ifdef BBMPC_REW_NPARAMS
                                                  , const float* __restrict__ params
#endif
                                                  ) {
    const int a = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_pop) return;
    const int HU = H * BBMPC_U;
    float c[BBMPC_S], nx[BBMPC_S], ac[BBMPC_U];
    for (int i = 0; i < BBMPC_S; ++i) c[i] = state[a * BBMPC_S + i];
    float total = 0.0f;
    for (int t = 0; t < H; ++t) {
        const float* row = traj + ((((size_t)t * A + a) * Nst) + n) * BBMPC_S;
        for (int i = 0; i < BBMPC_S; ++i) nx[i] = row[i];
        for (int u = 0; u < BBMPC_U; ++u) {
            const int j = t * BBMPC_U + u;
            ac[u] = from_ref ? seq[((size_t)n * A + a) * HU + j] : cand[((size_t)a * HU + j) * Nst + n];
        }
        total = total + BBMPC_CALL_REWARD(c, ac, nx, params, a, t);
        for (int i = 0; i < BBMPC_S; ++i) c[i] = nx[i];
    }
    if (total != total) total = -1.0e6f;
    rewards[(size_t)a * Nst + n] = total + rewards[(size_t)a * Nst + n];
}

// The particle evaluator over the learned model (bbmpc_set_particles, DESIGN.md section 8i): the TRAJ form of the MFMA
// particle rollout (kernels_mlp_particles.hpp) leaves the NOISY next state of every (candidate, particle) row and step in
// traj [H][A][S][RS], feature-major, the row's slot its returns index r = n * P + p.  One lane per row of agent blockIdx.y
// walks the horizon from the agent's state: consecutive lanes read consecutive floats of every feature.  The action is
// candidate n's, clipped HERE when `pen` (the particle path writes the feasible samples back only in the aggregate, behind
// this; kernels_particles.hpp particle_action).  Sum in index order, NaN -> -1e6 per particle, returns [A][RS].
extern "C" __global__ void bbmpc_user_reward_particles(int n_pop, int P, int A, int H, int Nst, int RS, int from_ref, int pen,
                                                       const float* __restrict__ state, const float* __restrict__ traj,
                                                       const float* __restrict__ seq, const float* __restrict__ cand,
                                                       const float* __restrict__ lo, const float* __restrict__ hi,
                                                       float* __restrict__ returns
#ifdef BBMPC_REW_NPARAMS
                                                       , const float* __restrict__ params
#endif
                                                       ) {
    const int a = blockIdx.y, r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_pop * P) return;
    const int n = r / P;
    const int HU = H * BBMPC_U;
    float c[BBMPC_S], nx[BBMPC_S], ac[BBMPC_U];
    for (int i = 0; i < BBMPC_S; ++i) c[i] = state[a * BBMPC_S + i];
    float total = 0.0f;
    for (int t = 0; t < H; ++t) {
        const float* tile = traj + (((size_t)t * A + a) * BBMPC_S) * RS + r;
        for (int i = 0; i < BBMPC_S; ++i) nx[i] = tile[(size_t)i * RS];
        for (int u = 0; u < BBMPC_U; ++u) {
            const int j = t * BBMPC_U + u;
            float v = from_ref ? seq[((size_t)n * A + a) * HU + j] : cand[((size_t)a * HU + j) * Nst + n];
            if (pen) v = (v < lo[u]) ? lo[u] : ((v > hi[u]) ? hi[u] : v);
            ac[u] = v;
        }
        total = total + BBMPC_CALL_REWARD(c, ac, nx, params, a, t);
        for (int i = 0; i < BBMPC_S; ++i) c[i] = nx[i];
    }
    if (total != total) total = -1.0e6f;
    returns[(size_t)a * RS + r] = total;
}

// Trajectory distributions (bbmpc_predict_trajectory_particles / _quantiles): k_traj_mlp_particles_kind leaves every
// particle state in pstates [B][P][Hq][S]; one lane per (b, p, t) fills prewards [B][P][Hq] from it -- the current state is
// row b's start state at t = 0 and pstates[b, p, t - 1] afterwards, no recurrence.  No clip and no NaN rule, as with a
// built-in reward.  Row b belongs to agent b / rows_per_agent, t is the step inside the sequence.
extern "C" __global__ void bbmpc_user_reward_traj_particles(int B, int P, int Hq, const float* __restrict__ states,
                                                            const float* __restrict__ seq, const float* __restrict__ pstates,
                                                            float* __restrict__ prewards
#ifdef BBMPC_REW_NPARAMS
                                                            , const float* __restrict__ params, int rows_per_agent
#endif
                                                            ) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * P * Hq) return;
    const int t = (int)(idx % Hq);
    const int b = (int)(idx / ((size_t)P * Hq));
    float c[BBMPC_S], nx[BBMPC_S], ac[BBMPC_U];
    for (int i = 0; i < BBMPC_S; ++i) {
        c[i] = t == 0 ? states[(size_t)b * BBMPC_S + i] : pstates[(idx - 1) * BBMPC_S + i];
        nx[i] = pstates[idx * BBMPC_S + i];
    }
    for (int u = 0; u < BBMPC_U; ++u) ac[u] = seq[((size_t)b * Hq + t) * BBMPC_U + u];
    prewards[idx] = BBMPC_CALL_REWARD(c, ac, nx, params, b / rows_per_agent, t);
}
)RTC";

static const char* const k_inverse_transform_rows_text = R"RTC(
// next = inverse_transform_targets_func(cur, dev) on rows (system_dynamics_handler.py:157-161)
extern "C" __global__ void bbmpc_user_inverse_transform_rows(const float* __restrict__ cur, const float* __restrict__ dev,
                                                             int batch, float* __restrict__ next) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float c[BBMPC_S], d[BBMPC_S], nx[BBMPC_S];
    for (int i = 0; i < BBMPC_S; ++i) { c[i] = cur[(size_t)b * BBMPC_S + i]; d[i] = dev[(size_t)b * BBMPC_S + i]; }
    bbmpc_user_inverse_transform_targets(c, d, nx, BBMPC_S);
    for (int i = 0; i < BBMPC_S; ++i) next[(size_t)b * BBMPC_S + i] = nx[i];
}
)RTC";

static const char* const k_transform_rows_text = R"RTC(
// target = transform_targets_func(cur, next) on rows (system_dynamics_handler.py:314)
extern "C" __global__ void bbmpc_user_transform_rows(const float* __restrict__ cur, const float* __restrict__ next,
                                                     int batch, float* __restrict__ target) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float c[BBMPC_S], nx[BBMPC_S], tg[BBMPC_S];
    for (int i = 0; i < BBMPC_S; ++i) { c[i] = cur[(size_t)b * BBMPC_S + i]; nx[i] = next[(size_t)b * BBMPC_S + i]; }
    bbmpc_user_transform_targets(c, nx, tg, BBMPC_S);
    for (int i = 0; i < BBMPC_S; ++i) target[(size_t)b * BBMPC_S + i] = tg[i];
}
)RTC";

static const char* const k_dynamics_rows_text = R"RTC(
extern "C" __global__ void bbmpc_user_dynamics_rows(const float* __restrict__ states, const float* __restrict__ act,
                                                    int astride, int batch, float* __restrict__ next_states
#ifdef BBMPC_DYN_NPARAMS
                                                    , const float* __restrict__ params, int rows_per_agent, int t
#endif
                                                    ) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float x[BBMPC_S + BBMPC_U], d[BBMPC_S];
    for (int i = 0; i < BBMPC_S; ++i) x[i] = states[(size_t)b * BBMPC_S + i];                    // process_input: concat
    for (int i = 0; i < BBMPC_U; ++i) x[BBMPC_S + i] = act[(size_t)b * astride + i];
    BBMPC_CALL_DYNAMICS(x, d, params, b / rows_per_agent, t);                                   // f(x, train=False) -> delta
#ifdef BBMPC_XFORM
    float nx[BBMPC_S];
    bbmpc_user_inverse_transform_targets(x, d, nx, BBMPC_S);                                    // the raw output (:148-151)
    for (int i = 0; i < BBMPC_S; ++i) next_states[(size_t)b * BBMPC_S + i] = nx[i];
#else
    for (int i = 0; i < BBMPC_S; ++i) next_states[(size_t)b * BBMPC_S + i] = d[i] + x[i];        // transforms.py:34
#endif
}
)RTC";

#include "_embed.inc"      // k_embed_fastmath, k_embed_models, k_embed_activations, k_embed_kernels_mlp_xform: headers as text (generated by _build.py)

// The FUSED form: one lane per candidate trajectory, the whole H-step recurrence in registers, with the user's
// function(s) inlined next to the built-in model / rewards (the engine's own models.hpp, compiled from the same text
// with the same flags).  Used whenever the dynamics is not the learned MLP (whose rollouts live on the matrix cores);
// the step-wise evaluator (kernels_user.hpp) stays for MLP + user reward.
//   BBMPC_DYN_KIND 1 = PendulumTrueModel (op-for-op form), 3 = bbmpc_user_dynamics
//   BBMPC_REW_KIND 1 / 2 = built-in pendulum / cheetah reward, 3 = bbmpc_user_reward
//   xform_src (user dynamics only, may be empty): the inverse target transform, inlined in place of next = delta + state
//   a parameterised side (BBMPC_REW_NPARAMS / BBMPC_DYN_NPARAMS): the kernel then takes rew_params / dyn_params [A][P]
//   after its classic arguments and hands the function the row of agent blockIdx.y -- uniform over the workgroup, so the
//   reads are scalar loads -- and the horizon step t
static const char* const k_rollout_text = R"RTC(
extern "C" __global__ void bbmpc_user_rollout(int n_pop, int A, int H, int Nst, int from_ref, int pen, int fix_q1,
                                              const float* __restrict__ state, const float* __restrict__ seq,
                                              const float* cand, float* samples, const float* __restrict__ lo,
                                              const float* __restrict__ hi, float* __restrict__ rewards,
                                              float* __restrict__ penalty_out
#if defined(BBMPC_REW_NPARAMS) || defined(BBMPC_DYN_NPARAMS)
                                              , const float* __restrict__ rew_params, const float* __restrict__ dyn_params
#endif
                                              ) {
    constexpr int S = BBMPC_S, U = BBMPC_U;
    const int a = blockIdx.y, n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_pop) return;
    const int HU = H * U;
    float x[S + U], nx[S];
    for (int i = 0; i < S; ++i) x[i] = state[a * S + i];                       // tf.tile(current_states, [nopt, 1])
    float total = 0.0f, pen_acc = 0.0f;
    for (int t = 0; t < H; ++t) {
        for (int u = 0; u < U; ++u) {
            const int j = t * U + u;
            float v = from_ref ? seq[((size_t)n * A + a) * HU + j] : cand[((size_t)a * HU + j) * Nst + n];
            if (pen) {
                const float xf = bbmpc::clipf(v, lo[u], hi[u]);
                const float d = v - xf;
                pen_acc = pen_acc + d * d;
                v = xf;
            }
            if (samples) samples[((size_t)a * HU + j) * Nst + n] = v;
            x[S + u] = v;
        }
#if BBMPC_DYN_KIND == 3
        {
            float d[S];
            BBMPC_CALL_DYNAMICS(x, d, dyn_params, a, t);                       // f(x, train=False) -> delta
#ifdef BBMPC_XFORM
            bbmpc_user_inverse_transform_targets(x, d, nx, S);                 // the raw output (:148-151)
#else
            for (int i = 0; i < S; ++i) nx[i] = d[i] + x[i];                     // transforms.py:34
#endif
        }
#else
        {
            float ss[3] = {x[0], x[1], x[2]};
            const float ac[1] = {x[3]};
            const bbmpc::PendulumModel model{fix_q1 != 0};
            (void)model.step(ss, ac);
            nx[0] = ss[0]; nx[1] = ss[1]; nx[2] = ss[2];
        }
#endif
#if BBMPC_REW_KIND == 3
        total = total + BBMPC_CALL_REWARD(x, x + S, nx, rew_params, a, t);      // (current_state, actions, next_state)
#else
        total = total + bbmpc::reward_generic(BBMPC_REW_KIND, fix_q1 != 0, x, x + S, nx, S, U);
#endif
        for (int i = 0; i < S; ++i) x[i] = nx[i];
    }
    if (total != total) total = -1.0e6f;                                         // deterministic.py:75-77
    if (pen) {
        const float nr = sqrtf(pen_acc);                                         // tf.norm(...)**2  pi2.py:72-75
        const float pv = nr * nr;
        total = total - pv;
        if (penalty_out) penalty_out[(size_t)a * Nst + n] = pv;
    }
    rewards[(size_t)a * Nst + n] = total;
}
)RTC";

// Open-loop trajectory prediction (bbmpc_predict_trajectories) for analytic models with a user function on either side:
// one lane per ROW of the batch, the Hq-step recurrence in registers as in bbmpc_user_rollout, but every row starts from
// its own state, every next state goes to states_out [B,Hq,S] and every step reward to rewards_out [B,Hq] (either may be
// null); no clip, no penalty, no NaN rule.  Row b belongs to agent b / rows_per_agent (parameterised sides), t is the step
// inside the sequence.  Same defines as the rollout.  Compiled on the handle's first prediction, never before.
static const char* const k_traj_text = R"RTC(
extern "C" __global__ void bbmpc_user_traj(int batch, int Hq, int fix_q1, const float* __restrict__ states,
                                           const float* __restrict__ seq, float* __restrict__ states_out,
                                           float* __restrict__ rewards_out
#if defined(BBMPC_REW_NPARAMS) || defined(BBMPC_DYN_NPARAMS)
                                           , const float* __restrict__ rew_params, const float* __restrict__ dyn_params,
                                           int rew_rows_per_agent, int dyn_rows_per_agent
#endif
                                           ) {
    constexpr int S = BBMPC_S, U = BBMPC_U;
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float x[S + U], nx[S];
    for (int i = 0; i < S; ++i) x[i] = states[(size_t)b * S + i];
    for (int t = 0; t < Hq; ++t) {
        for (int u = 0; u < U; ++u) x[S + u] = seq[((size_t)b * Hq + t) * U + u];
#if BBMPC_DYN_KIND == 3
        {
            float d[S];
            BBMPC_CALL_DYNAMICS(x, d, dyn_params, b / dyn_rows_per_agent, t);  // f(x, train=False) -> delta
#ifdef BBMPC_XFORM
            bbmpc_user_inverse_transform_targets(x, d, nx, S);                 // the raw output (:148-151)
#else
            for (int i = 0; i < S; ++i) nx[i] = d[i] + x[i];                     // transforms.py:34
#endif
        }
#else
        {
            float ss[3] = {x[0], x[1], x[2]};
            const float ac[1] = {x[3]};
            const bbmpc::PendulumModel model{fix_q1 != 0};
            (void)model.step(ss, ac);
            nx[0] = ss[0]; nx[1] = ss[1]; nx[2] = ss[2];
        }
#endif
        if (rewards_out) {
#if BBMPC_REW_KIND == 3
            rewards_out[(size_t)b * Hq + t] = BBMPC_CALL_REWARD(x, x + S, nx, rew_params, b / rew_rows_per_agent, t);
#else
            rewards_out[(size_t)b * Hq + t] = bbmpc::reward_generic(BBMPC_REW_KIND, fix_q1 != 0, x, x + S, nx, S, U);
#endif
        }
        if (states_out)
            for (int i = 0; i < S; ++i) states_out[((size_t)b * Hq + t) * S + i] = nx[i];
        for (int i = 0; i < S; ++i) x[i] = nx[i];
    }
}
)RTC";

// Compile for gfx950; returns the code object.  Throws std::runtime_error with the compiler log on failure.
inline std::vector<char> compile_rtc(const std::string& src, const char* name, const std::vector<std::string>& defines,
                                     bool with_engine_headers) {
    const Hiprtc& r = Hiprtc::get();
    Hiprtc::Program prog = nullptr;
    const char* hdr_text[] = {k_embed_fastmath, k_embed_models, k_embed_activations, k_embed_kernels_mlp_xform};
    const char* hdr_name[] = {"fastmath.hpp", "models.hpp", "activations.hpp", "kernels_mlp_xform.hpp"};
    int rc = r.CreateProgram(&prog, src.c_str(), name, with_engine_headers ? 4 : 0, with_engine_headers ? hdr_text : nullptr,
                             with_engine_headers ? hdr_name : nullptr);
    if (rc != 0) throw std::runtime_error(std::string("hiprtcCreateProgram: ") + r.GetErrorString(rc));
    // one rounding per source operation, as everywhere in the engine (and as the reference's TF ops round)
    std::vector<const char*> opts = {"--offload-arch=gfx950", "-O3", "-ffp-contract=off"};
    for (const std::string& d : defines) opts.push_back(d.c_str());
    rc = r.CompileProgram(prog, (int)opts.size(), opts.data());
    std::string log;
    size_t n = 0;
    if (r.GetProgramLogSize(prog, &n) == 0 && n > 1) {
        log.resize(n);
        (void)r.GetProgramLog(prog, &log[0]);
    }
    if (rc != 0) {
        (void)r.DestroyProgram(&prog);
        throw std::runtime_error(std::string("user device function failed to compile (") + r.GetErrorString(rc) + "):\n" + log);
    }
    std::vector<char> code;
    if (r.GetCodeSize(prog, &n) != 0 || n == 0) {
        (void)r.DestroyProgram(&prog);
        throw std::runtime_error("hiprtcGetCodeSize failed");
    }
    code.resize(n);
    rc = r.GetCode(prog, code.data());
    (void)r.DestroyProgram(&prog);
    if (rc != 0) throw std::runtime_error(std::string("hiprtcGetCode: ") + r.GetErrorString(rc));
    return code;
}

// The programs, numbered so that the four row programs keep their USER_KIND_* value.
constexpr int PROG_ROLLOUT = 5, PROG_MLP_XFORM_ROLLOUT = 6, PROG_TRAJ = 7;

// What a program is built from; each form reads the fields it needs (a row program: its own source and side; dynamics rows
// and the fused rollout: xform_src too; the learned-model transform rollout: xform_src, the reward side and act_ext).
struct UserProgram {
    int S = 0, U = 0;
    int dyn_kind = 0, rew_kind = 0;              // BBMPC_DYN_* / BBMPC_REW_* (3 = the user's function)
    std::string reward_src, dynamics_src;        // empty where that side is built in
    std::string xform_src;                       // the inverse target transform, or empty
    int rew_np = 0, dyn_np = 0;                  // > 0: that side is parameterised
    bool act_ext = true;                         // the network has an activation after sigmoid (activations.hpp): dispatch over every code
    // the source a row program (USER_KIND_*) is named after
    std::string& own_source(int kind) { return kind == USER_KIND_REWARD ? reward_src : kind == USER_KIND_DYNAMICS ? dynamics_src : xform_src; }
};

// the kernel a loaded program is entered by (the reward rows program also has bbmpc_user_reward_traj and the two particle
// scorers, bbmpc_user_reward_particles and bbmpc_user_reward_traj_particles)
inline const char* program_kernel(int form) {
    static const char* const names[] = {"", "bbmpc_user_reward_rows", "bbmpc_user_dynamics_rows", "bbmpc_user_inverse_transform_rows",
                                        "bbmpc_user_transform_rows", "bbmpc_user_rollout", "bbmpc_mlp_xform_rollout", "bbmpc_user_traj"};
    return names[form];
}

inline std::vector<std::string> program_defines(int form, const UserProgram& d) {
    std::vector<std::string> defs = {"-DBBMPC_S=" + std::to_string(d.S), "-DBBMPC_U=" + std::to_string(d.U)};
    if (form == PROG_ROLLOUT || form == PROG_TRAJ) defs.push_back("-DBBMPC_DYN_KIND=" + std::to_string(d.dyn_kind));
    if (form == PROG_ROLLOUT || form == PROG_MLP_XFORM_ROLLOUT || form == PROG_TRAJ) defs.push_back("-DBBMPC_REW_KIND=" + std::to_string(d.rew_kind));
    if (form == PROG_MLP_XFORM_ROLLOUT) defs.push_back(std::string("-DBBMPC_ACT_EXT=") + (d.act_ext ? "1" : "0"));
    const bool rew = form == USER_KIND_REWARD || form == PROG_ROLLOUT || form == PROG_MLP_XFORM_ROLLOUT || form == PROG_TRAJ;
    const bool dyn = form == USER_KIND_DYNAMICS || form == PROG_ROLLOUT || form == PROG_TRAJ;
    if (rew && d.rew_np > 0) defs.push_back("-DBBMPC_REW_NPARAMS=" + std::to_string(d.rew_np));
    if (dyn && d.dyn_np > 0) defs.push_back("-DBBMPC_DYN_NPARAMS=" + std::to_string(d.dyn_np));
    return defs;
}

inline std::string program_source(int form, const UserProgram& d) {
    const std::string xform = d.xform_src.empty() ? std::string()
        : "// ---- user inverse target transform ---------------------------------------------------\n" + d.xform_src + "\n#define BBMPC_XFORM 1\n";
    if (form == PROG_ROLLOUT || form == PROG_MLP_XFORM_ROLLOUT || form == PROG_TRAJ) {
        std::string s = "#include \"models.hpp\"\n";
        s += "// ---- user reward --------------------------------------------------------------------\n" + d.reward_src + "\n";
        if (form == PROG_MLP_XFORM_ROLLOUT) return s + xform + k_user_calls + "#define BBMPC_XFORM_KERNEL 1\n#include \"kernels_mlp_xform.hpp\"\n";
        s += "// ---- user dynamics ------------------------------------------------------------------\n" + d.dynamics_src + "\n";
        return s + xform + k_user_calls + (form == PROG_TRAJ ? k_traj_text : k_rollout_text);
    }
    std::string s = "// ---- user source ------------------------------------------------------------------\n";
    s += UserProgram(d).own_source(form) + "\n";
    if (form == USER_KIND_DYNAMICS) s += xform;
    s += "// ---- row kernels (blackbox_mpc_amd/csrc/rtc.hpp) ------------------------------------\n";
    s += k_user_calls;
    s += form == USER_KIND_REWARD ? k_reward_rows_text : form == USER_KIND_DYNAMICS ? k_dynamics_rows_text
         : form == USER_KIND_INVERSE_TRANSFORM ? k_inverse_transform_rows_text : k_transform_rows_text;
    return s;
}

// the code object of one program; only the two rollouts see the engine's headers (models.hpp, kernels_mlp_xform.hpp, ...)
inline std::vector<char> compile_program(int form, const UserProgram& d) {
    static const char* const names[] = {"", "bbmpc_user_reward.hip", "bbmpc_user_dynamics.hip", "bbmpc_user_inverse_transform.hip",
                                        "bbmpc_user_transform.hip", "bbmpc_user_rollout.hip", "bbmpc_mlp_xform_rollout.hip", "bbmpc_user_traj.hip"};
    return compile_rtc(program_source(form, d), names[form], program_defines(form, d), form >= PROG_ROLLOUT);
}

}  // namespace bbmpc
