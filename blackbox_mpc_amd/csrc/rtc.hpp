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
// calls).  The programs are then compiled with BBMPC_REW_NPARAMS / BBMPC_DYN_NPARAMS = P and the kernel texts below get
// the parameterised call and the extra kernel arguments filled in; a source without parameters gets exactly the classic
// text, so its kernels are the ones it always had.
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

// The kernel texts below carry @@NAME@@ slots where the classic and the parameterised programs differ; fill_slots puts
// one of the two in (every slot must be there: a missing one is a bug in this file, not in the user's source).
inline std::string fill_slots(std::string text, const std::vector<std::pair<std::string, std::string>>& slots) {
    for (const auto& kv : slots) {
        const std::string key = "@@" + kv.first + "@@";
        size_t at = text.find(key);
        if (at == std::string::npos) throw std::logic_error("rtc.hpp: kernel text without slot " + key);
        for (; at != std::string::npos; at = text.find(key, at + kv.second.size())) text.replace(at, key.size(), kv.second);
    }
    return text;
}

// The row kernels the engine launches around the user's function.  BBMPC_S / BBMPC_U are compile-time so the per-row
// arrays live in registers; rows are [batch, S] / [batch, astride] row-major.  `xform_src` (dynamics only, may be empty):
// the handle's inverse target transform, which then replaces next = delta + state (BBMPC_XFORM).  nparams > 0 (reward /
// dynamics): the parameterised entry point; the row kernels take (params [A][P], rows_per_agent, t) -- row b belongs to
// agent b / rows_per_agent -- and the traj scorer takes params and reads the row of agent blockIdx.y.
inline std::string user_program_source(const std::string& user_src, int kind, const std::string& xform_src = std::string(),
                                       int nparams = 0) {
    const bool par = nparams > 0;
    const char* const rows_args = par ? ",\n        const float* __restrict__ params, int rows_per_agent, int t" : "";
    std::string s;
    s += "// ---- user source ------------------------------------------------------------------\n";
    s += user_src;
    if (kind == USER_KIND_DYNAMICS && !xform_src.empty()) {
        s += "\n// ---- user inverse target transform ----------------------------------------------------\n";
        s += xform_src;
        s += "\n#define BBMPC_XFORM 1\n";
    }
    s += "\n// ---- row kernels (blackbox_mpc_amd/csrc/rtc.hpp) ------------------------------------\n";
    if (kind == USER_KIND_REWARD) {
        s += fill_slots(R"RTC(
extern "C" __global__ void bbmpc_user_reward_rows(const float* __restrict__ cur, const float* __restrict__ nxt,
                                                  const float* __restrict__ act, int astride, int batch,
                                                  float* __restrict__ total, int accumulate@@ROWS_ARGS@@) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float c[BBMPC_S], n[BBMPC_S], a[BBMPC_U];
    for (int i = 0; i < BBMPC_S; ++i) { c[i] = cur[(size_t)b * BBMPC_S + i]; n[i] = nxt[(size_t)b * BBMPC_S + i]; }
    for (int i = 0; i < BBMPC_U; ++i) a[i] = act[(size_t)b * astride + i];
    // reward_function(current_state, actions, next_state): the argument order of the CALL (deterministic.py:65-66)
    const float r = @@REWARD_ROW@@;
    total[b] = accumulate ? total[b] + r : r;
}

// The learned MLP's rollouts run on the matrix cores (kernels_mlp.hpp) and leave the state after every step in
// traj [H][A][Nst][S]; this scores the whole trajectory of one candidate per lane: sum_t r(s_t, a_t, s_t+1), NaN -> -1e6
// (deterministic.py:62-77).  `rewards` holds -(penalty) from the rollout kernel (0 without one): R - penalty.
extern "C" __global__ void bbmpc_user_reward_traj(int n_pop, int A, int H, int Nst, int from_ref,
                                                  const float* __restrict__ state, const float* __restrict__ traj,
                                                  const float* __restrict__ seq, const float* __restrict__ cand,
                                                  float* __restrict__ rewards@@TRAJ_ARGS@@) {
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
        total = total + @@REWARD_TRAJ@@;
        for (int i = 0; i < BBMPC_S; ++i) c[i] = nx[i];
    }
    if (total != total) total = -1.0e6f;
    rewards[(size_t)a * Nst + n] = total + rewards[(size_t)a * Nst + n];
}
)RTC",
                        {{"ROWS_ARGS", rows_args},
                         {"REWARD_ROW", par ? "bbmpc_user_reward_params(c, a, n, BBMPC_S, BBMPC_U, params + (size_t)(b / rows_per_agent) * "
                                              "BBMPC_REW_NPARAMS, t)"
                                            : "bbmpc_user_reward(c, a, n, BBMPC_S, BBMPC_U)"},
                         {"TRAJ_ARGS", par ? ", const float* __restrict__ params" : ""},
                         {"REWARD_TRAJ", par ? "bbmpc_user_reward_params(c, ac, nx, BBMPC_S, BBMPC_U, params + (size_t)a * BBMPC_REW_NPARAMS, t)"
                                             : "bbmpc_user_reward(c, ac, nx, BBMPC_S, BBMPC_U)"}});
    } else if (kind == USER_KIND_INVERSE_TRANSFORM) {
        s += R"RTC(
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
    } else if (kind == USER_KIND_TRANSFORM) {
        s += R"RTC(
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
    } else {
        s += fill_slots(R"RTC(
extern "C" __global__ void bbmpc_user_dynamics_rows(const float* __restrict__ states, const float* __restrict__ act,
                                                    int astride, int batch, float* __restrict__ next_states@@ROWS_ARGS@@) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    float x[BBMPC_S + BBMPC_U], d[BBMPC_S];
    for (int i = 0; i < BBMPC_S; ++i) x[i] = states[(size_t)b * BBMPC_S + i];                    // process_input: concat
    for (int i = 0; i < BBMPC_U; ++i) x[BBMPC_S + i] = act[(size_t)b * astride + i];
    @@DYNAMICS_ROW@@;                                                // f(x, train=False) -> delta
#ifdef BBMPC_XFORM
    float nx[BBMPC_S];
    bbmpc_user_inverse_transform_targets(x, d, nx, BBMPC_S);                                    // the raw output (:148-151)
    for (int i = 0; i < BBMPC_S; ++i) next_states[(size_t)b * BBMPC_S + i] = nx[i];
#else
    for (int i = 0; i < BBMPC_S; ++i) next_states[(size_t)b * BBMPC_S + i] = d[i] + x[i];        // transforms.py:34
#endif
}
)RTC",
                        {{"ROWS_ARGS", rows_args},
                         {"DYNAMICS_ROW", par ? "bbmpc_user_dynamics_params(x, d, BBMPC_S, BBMPC_U, params + (size_t)(b / rows_per_agent) * "
                                                "BBMPC_DYN_NPARAMS, t)"
                                              : "bbmpc_user_dynamics(x, d, BBMPC_S, BBMPC_U)"}});
    }
    return s;
}

#include "_embed.inc"      // k_embed_fastmath, k_embed_models, k_embed_activations, k_embed_kernels_mlp_xform: headers as text (generated by _build.py)

// The FUSED form: one lane per candidate trajectory, the whole H-step recurrence in registers, with the user's
// function(s) inlined next to the built-in model / rewards (the engine's own models.hpp, compiled from the same text
// with the same flags).  Used whenever the dynamics is not the learned MLP (whose rollouts live on the matrix cores);
// the step-wise evaluator (kernels_user.hpp) stays for MLP + user reward.
//   BBMPC_DYN_KIND 1 = PendulumTrueModel (op-for-op form), 3 = bbmpc_user_dynamics
//   BBMPC_REW_KIND 1 / 2 = built-in pendulum / cheetah reward, 3 = bbmpc_user_reward
//   xform_src (user dynamics only, may be empty): the inverse target transform, inlined in place of next = delta + state
//   rew_np / dyn_np > 0: that side is parameterised (BBMPC_REW_NPARAMS / BBMPC_DYN_NPARAMS); the kernel then takes
//   rew_params / dyn_params [A][P] after its classic arguments and hands the function the row of agent blockIdx.y --
//   uniform over the workgroup, so the reads are scalar loads -- and the horizon step t
inline std::string user_rollout_source(const std::string& reward_src, const std::string& dynamics_src,
                                       const std::string& xform_src = std::string(), int rew_np = 0, int dyn_np = 0) {
    std::string s = "#include \"models.hpp\"\n";
    s += "// ---- user reward --------------------------------------------------------------------\n" + reward_src + "\n";
    s += "// ---- user dynamics ------------------------------------------------------------------\n" + dynamics_src + "\n";
    if (!xform_src.empty())
        s += "// ---- user inverse target transform ---------------------------------------------------\n" + xform_src + "\n#define BBMPC_XFORM 1\n";
    s += fill_slots(R"RTC(
extern "C" __global__ void bbmpc_user_rollout(int n_pop, int A, int H, int Nst, int from_ref, int pen, int fix_q1,
                                              const float* __restrict__ state, const float* __restrict__ seq,
                                              const float* cand, float* samples, const float* __restrict__ lo,
                                              const float* __restrict__ hi, float* __restrict__ rewards,
                                              float* __restrict__ penalty_out@@PARAM_ARGS@@) {
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
            @@DYNAMICS_STEP@@;                                   // f(x, train=False) -> delta
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
        total = total + @@REWARD_STEP@@;                   // (current_state, actions, next_state)
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
)RTC",
                    {{"PARAM_ARGS", rew_np > 0 || dyn_np > 0 ? ",\n        const float* __restrict__ rew_params, const float* __restrict__ dyn_params" : ""},
                     {"DYNAMICS_STEP", dyn_np > 0 ? "bbmpc_user_dynamics_params(x, d, S, U, dyn_params + (size_t)a * BBMPC_DYN_NPARAMS, t)"
                                                  : "bbmpc_user_dynamics(x, d, S, U)"},
                     {"REWARD_STEP", rew_np > 0 ? "bbmpc_user_reward_params(x, x + S, nx, S, U, rew_params + (size_t)a * BBMPC_REW_NPARAMS, t)"
                                                : "bbmpc_user_reward(x, x + S, nx, S, U)"}});
    return s;
}

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

// the -D flags of a parameterised side (none for a classic source)
inline void add_nparams_defines(std::vector<std::string>& defs, int rew_np, int dyn_np) {
    if (rew_np > 0) defs.push_back("-DBBMPC_REW_NPARAMS=" + std::to_string(rew_np));
    if (dyn_np > 0) defs.push_back("-DBBMPC_DYN_NPARAMS=" + std::to_string(dyn_np));
}

inline std::vector<char> compile_user_program(const std::string& user_src, int kind, int S, int U,
                                             const std::string& xform_src = std::string(), int nparams = 0) {
    static const char* const names[] = {"", "bbmpc_user_reward.hip", "bbmpc_user_dynamics.hip", "bbmpc_user_inverse_transform.hip",
                                        "bbmpc_user_transform.hip"};
    std::vector<std::string> defs = {"-DBBMPC_S=" + std::to_string(S), "-DBBMPC_U=" + std::to_string(U)};
    add_nparams_defines(defs, kind == USER_KIND_REWARD ? nparams : 0, kind == USER_KIND_DYNAMICS ? nparams : 0);
    return compile_rtc(user_program_source(user_src, kind, xform_src, nparams), names[kind], defs, false);
}

inline std::vector<char> compile_user_rollout(const std::string& reward_src, const std::string& dynamics_src, int dyn_kind, int rew_kind,
                                              int S, int U, const std::string& xform_src = std::string(), int rew_np = 0, int dyn_np = 0) {
    std::vector<std::string> defs = {"-DBBMPC_S=" + std::to_string(S), "-DBBMPC_U=" + std::to_string(U),
                                     "-DBBMPC_DYN_KIND=" + std::to_string(dyn_kind), "-DBBMPC_REW_KIND=" + std::to_string(rew_kind)};
    add_nparams_defines(defs, rew_np, dyn_np);
    return compile_rtc(user_rollout_source(reward_src, dynamics_src, xform_src, rew_np, dyn_np), "bbmpc_user_rollout.hip", defs, true);
}

// The learned-model rollout with the inverse target transform inlined (kernels_mlp_xform.hpp); reward_src is the user
// reward when rew_kind == 3 (BBMPC_REW_USER), else empty and a built-in reward kind.
inline std::string mlp_xform_rollout_source(const std::string& xform_src, const std::string& reward_src) {
    std::string s = "#include \"models.hpp\"\n";
    s += "// ---- user reward --------------------------------------------------------------------\n" + reward_src + "\n";
    s += "// ---- user inverse target transform ---------------------------------------------------\n" + xform_src + "\n";
    s += "#define BBMPC_XFORM_KERNEL 1\n#include \"kernels_mlp_xform.hpp\"\n";
    return s;
}

// act_ext: the network has an activation after sigmoid (activations.hpp), so the program dispatches over every code.
// rew_np > 0: a parameterised user reward (the kernel then takes rew_params [A][P] after XformArgs).
inline std::vector<char> compile_mlp_xform_rollout(const std::string& xform_src, const std::string& reward_src, int rew_kind, int S, int U,
                                                   bool act_ext = true, int rew_np = 0) {
    std::vector<std::string> defs = {"-DBBMPC_S=" + std::to_string(S), "-DBBMPC_U=" + std::to_string(U),
                                     "-DBBMPC_REW_KIND=" + std::to_string(rew_kind), std::string("-DBBMPC_ACT_EXT=") + (act_ext ? "1" : "0")};
    add_nparams_defines(defs, rew_np, 0);
    return compile_rtc(mlp_xform_rollout_source(xform_src, reward_src), "bbmpc_mlp_xform_rollout.hip", defs, true);
}

struct UserFunction {
    std::string source;
    int nparams = 0;                       // > 0: the source defines the parameterised entry point (bbmpc_set_*_source_params)
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    hipFunction_t fn_traj = nullptr;       // reward module only: bbmpc_user_reward_traj
    bbmpc_rows_callback cb = nullptr;      // or: a host callback working on device memory (bbmpc_set_*_callback)
    void* cb_user = nullptr;
    bool ready() const { return fn != nullptr || cb != nullptr; }
    void release() {
        if (module) (void)hipModuleUnload(module);
        module = nullptr;
        fn = nullptr;
        fn_traj = nullptr;
    }
};

}  // namespace bbmpc
