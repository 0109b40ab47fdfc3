// Host-side engine behind the C ABI: owns device memory, the stream, RNG step
// counter, injected-noise buffers and traces, and enqueues the per-control-step
// kernel sequence of each optimizer.
#pragma once
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/bbmpc.h"
#include "comm.hpp"
#include "completion_line.hpp"
#include "kernels_cma.hpp"
#include "kernels_eigh.hpp"
#include "kernels_eigh_small.hpp"
#include "kernels_fused.hpp"
#include "kernels_fused_cma.hpp"
#include "kernels_fused_pso.hpp"
#include "kernels_mlp.hpp"
#include "kernels_mlp_xform.hpp"
#include "kernels_mlp_q4s.hpp"
#include "kernels_mlp_w4.hpp"
#include "kernels_mlp_wave.hpp"
#include "kernels_opt.hpp"
#include "kernels_plan_grad.hpp"
#include "kernels_plan_refine.hpp"
#include "kernels_refit.hpp"
#include "kernels_reward_mlp.hpp"
#include "kernels_rollout.hpp"
#include "kernels_tail.hpp"
#include "kernels_user.hpp"

namespace bbmpc {

struct ParticleArgs;       // kernels_particles.hpp
struct TrajParticleArgs;   // kernels_traj_particles.hpp
struct MlpLaunch;          // bbmpc_mlp.hip

struct HipError : std::runtime_error {
    int code;
    HipError(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};

#define HIP_CHECK(expr)                                                                          \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            throw HipError(BBMPC_E_HIP, std::string(#expr) + " failed: " + hipGetErrorString(_e) + \
                                            " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

#define REQUIRE(cond, code, msg) \
    do {                         \
        if (!(cond)) throw HipError((code), (msg)); \
    } while (0)

template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    void alloc(size_t count) {
        release();
        n = count;
        if (count) HIP_CHECK(hipMalloc((void**)&p, count * sizeof(T)));
    }
    void zero(hipStream_t s) {
        if (p) HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), s));
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
};

hipStream_t masked_stream_from_env(const char* name, int cu_count);

// A user-supplied function as the handle holds it: a program compiled at run time (rtc.hpp, loaded by bbmpc_user.hip) or
// a host callback.
struct UserProgram;
struct UserFunction {
    std::string source;
    int nparams = 0;                       // > 0: the source defines the parameterised entry point (bbmpc_set_*_source_params)
    hipModule_t module = nullptr;
    hipFunction_t fn = nullptr;
    hipFunction_t fn_traj = nullptr;       // reward module only: bbmpc_user_reward_traj
    hipFunction_t fn_particles = nullptr;       // ... bbmpc_user_reward_particles (the particle rollout's scorer)
    hipFunction_t fn_traj_particles = nullptr;  // ... bbmpc_user_reward_traj_particles (the trajectory distribution's)
    bbmpc_rows_callback cb = nullptr;      // or: a host callback working on device memory (bbmpc_set_*_callback)
    void* cb_user = nullptr;
    void release() {
        if (module) (void)hipModuleUnload(module);
        module = nullptr;
        fn = nullptr;
        fn_traj = nullptr;
        fn_particles = nullptr;
        fn_traj_particles = nullptr;
    }
};

// The hand-off between the caller of a control step and the step's last kernel: the caller asks (engine_util.hpp:
// TailRequest) either for a sequence number that the kernel publishes itself when the record is complete
// (RecordComm::flag, or the host-polled completion word host_done) or for a completion event on the kernel's dispatch
// packet; the launch site that can serve the request takes it and marks it attached.  Empty outside a request.
struct TailHandoff {
    uint32_t* flag = nullptr;      // where the last kernel publishes `value`
    uint32_t* count = nullptr;     // arrival counter that goes with flag (device memory)
    uint32_t value = 0;
    hipEvent_t event = nullptr;    // or: completion event wanted on the last kernel (launch_with_tail)
    bool attached = false;         // the step's last kernel took the request
    // launch sites whose argument struct carries the three words
    template <class KernelArgs>
    void publish_into(KernelArgs& x) {
        if (flag) { x.done_flag = flag; x.done_count = count; x.done_value = value; attached = true; }
    }
    // ... and those whose kernel takes them as trailing arguments
    struct Words { uint32_t* flag; uint32_t* count; uint32_t value; };
    Words publish_words() {
        if (flag) attached = true;
        return {flag, count, value};
    }
};

struct Engine {
    bbmpc_config cfg;
    int N, A, H, U, S, HU, Nst, iters, k;
    int rec;                 // record width U+S+1
    std::vector<float> lo, hi;
    hipStream_t own_stream = nullptr, stream = nullptr;
    int cu_count = 0;        // its compute units (kernels with spinning barriers are sized against it)
    int device = 0;          // the device the handle lives on (cfg.device, or the caller's current device when that is < 0)
    uint32_t step_counter = 0;
    // A steady-state control step of the learned-model PI2 / CEM path replayed as a hipGraph (bbmpc_optimize): its eleven
    // dependent launches follow each other ~1 us closer than enqueued one by one (tools/microbench/launch_chain.hip:
    // 2.9 us per tiny dependent kernel on a stream, 1.95 us as a graph).  The launch arguments are frozen at capture; the two
    // words that change per call -- the control step the draws are keyed by and the completion value the tail publishes --
    // are read by the kernels from device memory that the step's last kernel advances (and the host re-synchronises
    // after calls that did not go through the graph).
    hipGraphExec_t step_graph = nullptr;
    uint64_t step_graph_sig = 0;           // what the graph was captured for (mutation count, exploration-noise flag)
    uint64_t step_warm_sig = 0;            // ... and what the current run of identical calls looks like
    int step_graph_warm = 0;               // consecutive eligible calls that ran the steady-state launch sequence
    uint32_t mutations = 0;                // bumped by everything that can change what a control step launches
    uint32_t* step_words_dev = nullptr;    // device memory: [0] control step, [1] completion value, [2] arrival counter of the tail's workgroups
    uint32_t* step_words = nullptr;        // pinned staging for re-synchronising them
    uint32_t step_mirror[2] = {0, 0};      // what the device words hold now
    void ensure_step_words();              // allocates step_words / step_words_dev on first use
    bool step_capturing = false;
    int64_t calls_graph = 0;               // replays so far (bbmpc_graph_stats)
    int64_t graph_capture_failures = 0;    // captures / instantiations that failed (the handle then stops trying)
    bool last_step_steady = false;         // the last optimize_dev ran without k_dist_init (kernels as they will be replayed)
    void invalidate_step_graph() {
        ++mutations;
        step_graph_warm = 0;
        if (step_graph) { (void)hipGraphExecDestroy(step_graph); step_graph = nullptr; }
    }
    bool trace_on = false, profiling = false;
    int prof_every = 1;      // events around every prof_every-th launch of the dominant kernel
    uint64_t prof_seq = 0;
    bool prof_this = false;
    int fused_mode = -1;     // -1 auto, 0 never, 1 always (env BBMPC_FUSED)
    // development / parity switches, read from the environment ONCE when the handle is created
    struct Switches {
        bool cma_svd_v1 = false, cma_svd_rounds = false, cma_svd_general = false, cma_svd_gram = false, cma_fused = false, cma_coop = false;
        bool cma_eigh_fail = false;    // BBMPC_CMA_EIGH_FAIL: test hook, the direct solver reports every instance as failed
        int cma_eigh = 1;              // BBMPC_CMA_EIGH=0: block Jacobi instead of the direct eigensolver (kernels_eigh.hpp) at 128 < n <= 320
        int cma_nb = 0;                // BBMPC_CMA_NB: 8 / 16 column blocks in the block Jacobi (0 = automatic)   // BBMPC_CMA_SVD_V1 / _ROUNDS / _GENERAL
        bool mlp_generic = false;      // BBMPC_MLP_GENERIC
        int mlp_bf16 = 0;              // BBMPC_MLP_BF16: 0 off (default, fp32), 1 plain bf16 inputs, 3 split bf16 (hi+lo, three products)
        int mlp_pair = -1, mlp_q4 = -1;   // BBMPC_MLP_PAIR / BBMPC_MLP_Q4: -1 automatic, 0 / 1 forced
        int mlp_w4 = 1;                   // BBMPC_MLP_W4=0: keep k_rollout_mlp_wave where k_rollout_mlp_w4 (hidden <= 32) would run
        int mlp_q4s = 1;                  // BBMPC_MLP_Q4S=0 (and the older spelling BBMPC_MLP_Q4R=0): keep k_rollout_mlp_q4 where k_rollout_mlp_q4s would run
        int cma_small3 = 1;               // BBMPC_CMA_SMALL3=0: n <= 32 keeps one launch per phase (eleven per iteration) instead of sample | roll out | update
        int step_graph = 1;               // BBMPC_STEP_GRAPH=0: never replay a control step as a hipGraph
        int pi2_skip_init = 1;            // BBMPC_PI2_SKIP_INIT=0: k_dist_init opens every PI2 / CEM control step on the learned-model path too
        int refit_wgs = 0;                // BBMPC_REFIT_WGS=n: workgroups per agent in k_refit_cem_v2 (0 = by problem size)
        int mlp_wave = 1;                 // BBMPC_MLP_WAVE=0: never the one-wave-per-tile kernel for small networks
        int linger_us = 200;              // BBMPC_LINGER_US: how long a one-agent control-step kernel waits for the next call (0 = never)
        int fused_bound = 0;              // BBMPC_FUSED_BOUND: 512 / 1024 = the launch bound of k_fused_pendulum where both forms exist (1024: the
                                          // 1024-thread form at every size), 0 = unset: 512 wherever the workgroup fits it
        int cem_wave_select = 1;          // BBMPC_CEM_WAVE_SELECT=0: the 512-thread CEM control step keeps the selection with wave 0's scan and the
                                          // shared elite list (csrc/topk.hpp) where the all-wave route would run; read when the handle is created
        bool trace_select_only = false;   // BBMPC_TRACE_SELECT_ONLY: test hook, bbmpc_set_trace leaves the persistent pendulum kernel's sorted-elites
                                          // trace out, so that its selection takes the route it takes untraced (BBMPC_TRACE_TOPK_PASSES bit 8)
        int balance = 0;               // BBMPC_BALANCE: parsed, ignored (the rollout's pacing of SIMD mates was taken out)
        int ilp = 1;                   // BBMPC_ILP
        bool refit_v1 = false;         // BBMPC_REFIT_V1
        bool zero_copy = true;         // !BBMPC_NO_ZERO_COPY
        bool mlp_no_half_tail = false; // BBMPC_MLP_NO_HALF_TAIL: keep hidden features in index order (no skipped MFMAs)
        bool host_poll = true;         // !BBMPC_NO_HOST_POLL: host calls return on the kernel's own completion word
        bool prof_reward_mlp = false;  // BBMPC_PROF_REWARD_MLP: bbmpc_set_profiling brackets k_reward_mlp_traj instead of the rollout kernel in front of it
        bool dbg = false;              // BBMPC_DBG
    } sw;

    // device state
    DevBuf<float> d_lo, d_hi, d_state, d_record, d_action;
    DevBuf<float> d_prev_mean, d_var0, d_mean, d_var, d_sigma;
    DevBuf<float> d_samples, d_rewards, d_penalty;
    DevBuf<int> d_elites;
    // learned dynamics (bbmpc_set_mlp)
    bool mlp_ready = false;
    MlpDesc mlp;
    int mlp_nw = 1;
    DevBuf<float> d_wpack[MLP_MAX_LAYERS], d_wpack4[MLP_MAX_LAYERS], d_bpack[MLP_MAX_LAYERS], d_wraw[MLP_MAX_LAYERS], d_braw[MLP_MAX_LAYERS], d_wq4[MLP_MAX_LAYERS], d_wq4s0, d_w4pack, d_wbf[MLP_MAX_LAYERS], d_stats;
    DevBuf<float> d_fin_next, d_fin_rew, d_step_act;
    // SPSA / PSO state (internal layout)
    DevBuf<float> d_cand_a, d_cand_b, d_rewards2, d_vel, d_pbest, d_pbest_r, d_gbest, d_gbest_r, d_cond;
    DevBuf<int> d_gidx;
    DevBuf<float> t_rewards2;
    bool pso_seeded = false;
    // CMA-ES state
    int cma_G = 0, cma_n = 0;
    CmaConst cma_c;
    DevBuf<float> c_w, c_m, c_sigma, c_C, c_B, c_Dd, c_ps, c_pc, c_BD, c_z, c_Ye, c_xm, c_ym, c_evec, c_eval, c_E;
    DevBuf<int> c_eidx, c_info;
    DevBuf<unsigned> c_sync;       // SVD instance barriers / sweep flags [G][32]
    // direct eigensolver scratch (kernels_eigh.hpp): tridiagonal, reflectors, eigenvectors in the tridiagonal basis, flags
    DevBuf<float> e_d, e_e, e_tau, e_Vt, e_alpha, e_lam, e_Z, e_Z2, e_P, e_Tf;
    DevBuf<unsigned> e_flags;
    // the one-workgroup direct solver of kernels_eigh_small.hpp
    bool cma_use_eigh_small() const { return sw.cma_eigh && cma_n >= 2 && cma_n <= ES_N && !sw.cma_svd_v1 && !sw.cma_svd_rounds && !sw.cma_svd_general && !sw.cma_svd_gram; }
    bool cma_use_eigh() const { return sw.cma_eigh && cma_n > 128 && cma_n <= EIGH_MAX_N && (cma_n & 3) == 0 && !sw.cma_svd_v1 && !sw.cma_svd_rounds && !sw.cma_svd_general && !sw.cma_svd_gram; }
    void cma_eigh_launch(const CmaArgs& q);
    // experiment switch BBMPC_EIGH_SIDE_CUS=lo-hi: the tridiagonalisation on a side stream confined to those CUs (event hand-offs)
    hipStream_t eigh_side = nullptr;
    hipEvent_t eigh_ev[2] = {nullptr, nullptr};
    int eigh_side_state = -1;         // -1 undecided, 0 off, 1 on
    DevBuf<float> d_eval_rew, d_step_c;    // evaluate_dev / step_dev scratch (grown on demand)
    DevBuf<float> d_stage;                 // the one staging buffer of the host-in / host-out calls (abi_util.hpp HostStage): no _dev member touches it
    int stage_depth = 0;                   // ... and how many stages are live (a nested one keeps a buffer of its own)
    // injected noise (internal layout), keyed by BBMPC_NOISE_*
    std::map<int, DevBuf<float>> inj;
    // traces
    DevBuf<float> t_rewards, t_mean, t_var, t_samples;
    DevBuf<int> t_elites;
    DevBuf<int> t_passes;          // [iters][A] radix passes of the CEM elite selection (BBMPC_TRACE_TOPK_PASSES)
    DevBuf<int> t_cma_stats;                     // [iters][G][16] BBMPC_TRACE_CMA_SVD_STATS
    DevBuf<float> t_cma_B, t_cma_C, t_cma_D;   // CMA-ES: eigenvectors / covariance / sqrt eigenvalues after each iteration
    // pinned staging
    float* h_pin = nullptr;
    float* h_pin_dev = nullptr;   // device address of h_pin (looked up once per allocation)
    size_t h_pin_n = 0;
    // noise prefetch for the persistent kernel: the standard draws of control step t+1 are generated by otherwise
    // idle CUs on a side stream while step t's kernel runs (same Philox counters => bit-identical to in-kernel draws)
    DevBuf<float> d_noise_pf[2];      // two chunks of pf_steps control steps each
    RecordComm rc;           // multi-GPU record all-gather (comm.hpp); unused until bbmpc_comm_init
    DevBuf<float> d_record_slot[RecordComm::kSlots];   // bbmpc_optimize_gather: the all-gather of step t reads its records while step t+1 runs
    float* h_record_stage[RecordComm::kSlots] = {nullptr, nullptr};   // pinned: the rank's records on their way host -> HBM (communication stream)
    // bbmpc_optimize_gather enqueues the collective of a control step while the NEXT one runs on the GPU (its ~20 us of
    // host API time would otherwise sit between two control steps): staged records whose gather is not enqueued yet
    bool gather_deferred[RecordComm::kSlots] = {false, false};
    float* gather_deferred_dst[RecordComm::kSlots] = {nullptr, nullptr};
    void (*settle_hook)(Engine*) = nullptr;      // flushes them when anything settles the handle
    void (*in_flight_hook)(Engine*) = nullptr;   // called once per host-in / host-out control step, right after it was handed to the GPU
    bool in_flight_called = false;
    void note_in_flight() { if (in_flight_hook && !in_flight_called) { in_flight_called = true; in_flight_hook(this); } }
    TailHandoff tail;                  // what the caller of optimize_dev wants from the control step's last kernel (TailRequest installs it)
    // host-in/host-out calls of a single-kernel control step return as soon as the kernel has published its records
    // into host memory; the stream is joined lazily by the next call that needs it (settle)
    uint32_t* host_done = nullptr;     // pinned host word the kernel publishes to
    uint32_t* host_done_dev = nullptr; // its device address
    uint32_t* host_count = nullptr;    // device memory arrival counter
    uint32_t host_seq = 0;
    void ensure_completion_block();    // allocates host_done / host_count on first use
    bool lazy_sync = false;
    void settle();
    // resident control-step kernel (one agent, persistent pendulum kernel, host-in / host-out calls): the kernel of one
    // call stays on the GPU for linger_us and takes the next call's request from a pinned mailbox line (kernels_fused.hpp)
    const float* stage_state_src = nullptr;   // pinned [A,S] state that the control step's first kernel (k_dist_init) copies to d_state
    bool linger_launch = false;        // bbmpc_optimize asks optimize_fused for the LINGER variant
    bool resident_alive = false;       // a LINGER kernel may still be polling the mailbox
    // pinned block host_done, 16-word lines: 0 completion word of the launch-per-call paths | 1..A per-agent completion
    // lines of the resident kernel (completion_line.hpp: the record's ten half-words, each tagged with the low 16 bits of
    // the call's sequence number, and the whole number in word 15 -- the line IS the record, the kernel writes no other) |
    // A+1..2A request lines | 2A+1..3A exit words | 3A+1.. agent map of a subset launch (one int32 per agent: ceil(A/16)
    // lines -- every agent but one may be listed)
    static constexpr int kLingerMaxAgents = 64;
    int sync_lines() const {
        const int al = std::max(1, std::min(A, kLingerMaxAgents));
        return 1 + 3 * al + (al + 15) / 16;
    }
    uint32_t* ack_host(int a) { return host_done + 16 * (1 + a); }
    uint32_t* mbox_host(int a) { return host_done + 16 * (1 + std::min(A, kLingerMaxAgents) + a); }
    uint32_t* gone_host(int a) { return host_done + 16 * (1 + 2 * std::min(A, kLingerMaxAgents) + a); }
    int32_t* amap_host() { return reinterpret_cast<int32_t*>(host_done + 16 * (1 + 3 * std::min(A, kLingerMaxAgents))); }
    uint32_t* sync_dev(const void* host_ptr) { return host_done_dev + (reinterpret_cast<const uint32_t*>(host_ptr) - host_done); }
    // Another handle of the process starting work on the same device asks the resident workgroups of this one to leave
    // (streams share a few hardware queues: a lingering kernel would hold back whatever lands behind it): it writes the stop
    // word into the request lines published here, nothing else -- this handle finds the exit words at its next call.
    std::atomic<uint32_t*> mbox_pub{nullptr};      // request lines of a (possibly) live resident kernel, null otherwise
    int mbox_pub_agents = 0;
    int subset_n = 0;                  // > 0: the next persistent-kernel launch covers only the agents listed in amap_host()
    int linger_test_quit = -1;         // BBMPC_LINGER_TEST_QUIT (test hook, kernels_fused.hpp)
    int64_t calls_resident = 0, calls_launched = 0;   // bbmpc_call_stats
    bool resident_step(const float* state, int add_noise, uint32_t seq, float* records);   // records: [A][5], decoded from the completion lines
    void resident_stop();
    hipStream_t pf_stream = nullptr;
    hipEvent_t pf_done[2] = {nullptr, nullptr}, pf_free = nullptr;
    int64_t pf_chunk[2] = {-1, -1};   // chunk id (control step / pf_steps) a buffer holds
    bool pf_waited[2] = {false, false}, pf_inflight[2] = {false, false};
    int pf_steps = 0;                 // control steps per chunk
    size_t pf_step_floats = 0;        // floats per control step
    int pf_mode = -1;                 // -1 undecided, 0 off, 1 on (env BBMPC_NOISE_PREFETCH)
    void launch_noise_fill(int64_t chunk, int buf, hipStream_t on);
    // profiling
    std::vector<hipEvent_t> ev_pool;
    size_t ev_used = 0;
    const char* dominant_kernel = "k_rollout_pendulum";
    // the template instantiation of the dominant kernel that the last control step launched, spelt the way rocprofv3 prints
    // kernel names (minus "void "): the key bench.py matches the committed PMC profiles on.  Empty = the plain name is unique.
    char dominant_inst[128] = "";

    explicit Engine(const bbmpc_config& c);
    ~Engine();

    RngKey key(uint32_t step) const {
        RngKey kk;
        kk.k0 = (uint32_t)(cfg.seed & 0xffffffffu);
        kk.k1 = (uint32_t)(cfg.seed >> 32);
        kk.step = step;
        kk.q_per_agent = (uint32_t)((HU + 3) / 4);
        kk.step_src = step_capturing ? step_words_dev : nullptr;
        return kk;
    }
    bool fix(uint32_t bit) const { return (cfg.quirks & bit) != 0; }
    // user-supplied reward / dynamics device functions and the step-wise evaluator that calls them (bbmpc_user.hip; kind =
    // rtc.hpp's USER_KIND_*)
    UserFunction user_reward, user_dynamics, user_rollout;   // user_rollout: the fused lane-per-trajectory kernel (rtc.hpp), built lazily
    bool user_rollout_stale = true;
    bool user_stepwise_only = false;   // BBMPC_USER_STEPWISE: never fuse (test / comparison hook)
    void rollout_user_fused(int mode, bool pen, RolloutArgs& ra);
    void rollout_mlp_user_reward(int mode, bool pen, RolloutArgs& ra);
    DevBuf<float> u_traj;              // [H][A][Nst][S] states after every step of the MFMA rollout
    // set around a launch_rollout_mlp call whose state argument is the pinned host buffer: a kernel that can store the
    // state for the later launches itself (k_rollout_mlp_q4s) takes the request and clears it.  A member and not an
    // argument because the request crosses launch_rollout's routing between first_rollout_mlp and launch_rollout_mlp
    float* mlp_state_copy = nullptr;
    bool pi2_dist_ready = false;       // d_sigma holds the constructor variance's root (PI2 never changes it)
    bool pi2_copy_seen = false;        // the previous control step's first rollout took such a request
    bool cem_sigma0_ready = false;     // d_sigma0 holds cem_sigma(prev_mean, var0): constant while CEM restarts from the constructor distribution
    DevBuf<float> d_sigma0;
    DevBuf<float> u_rows, u_x0, u_x1, u_total, u_pen, u_next;
    // target transforms (rtc.hpp USER_KIND_*TRANSFORM): the inverse one replaces next = dev + state in every dynamics step of
    // the handle, so a handle with one takes the user-function paths; the forward one only serves bbmpc_transform_rows
    UserFunction user_xform, user_fwd_xform, user_xform_rollout;   // user_xform_rollout: kernels_mlp_xform.hpp, built lazily
    bool user_xform_rollout_stale = true;
    bool user_xform_rollout_ext = false;     // the program was compiled for a network with an activation after sigmoid
    bool has_xform() const { return !user_xform.source.empty(); }
    void set_transform_source(int kind, const char* src);
    void transform_rows(int kind, const float* d_a, const float* d_b, int batch, float* d_out);
    void rollout_mlp_xform(int mode, bool pen, RolloutArgs& ra);
    void mlp_xform_rows(const float* d_states, const float* d_actions, int astride, int batch, float* d_next);
    DevBuf<float> u_xin, u_xraw;       // learned model + transform, step-wise: processed inputs / de-normalised outputs
    // (a learned reward model, BBMPC_REW_MLP, is routed exactly as a HIP-source reward over the learned model is)
    bool user_path() const { return cfg.reward == BBMPC_REW_USER || cfg.reward == BBMPC_REW_MLP || cfg.dynamics == BBMPC_DYN_USER || has_xform(); }
    int builtin_reward_kind() const { return (cfg.reward == BBMPC_REW_USER || cfg.reward == BBMPC_REW_MLP) ? REW_NONE : cfg.reward; }
    // learned reward model (bbmpc_set_reward_mlp; bbmpc_mlp.hip, kernels_reward_mlp.hpp): the MFMA
    // rollout records the trajectory as for a HIP-source reward, k_reward_mlp_traj + k_reward_mlp_finish score it; the
    // one-step calls and bbmpc_predict_trajectories go through k_reward_mlp_rows
    bool rew_mlp_ready = false;
    RewMlpDesc rew_mlp;
    DevBuf<float> d_rw_wp4[MLP_MAX_LAYERS], d_rw_bp[MLP_MAX_LAYERS], d_rw_last, d_rw_stats, d_rw_step, d_rw_states;
    void set_reward_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b, int input_mask,
                        int is_normalized, const float* const* stats);
    void rollout_mlp_reward_mlp(int mode, bool pen, RolloutArgs& ra, bool finish = true);   // finish = false: the step rewards stay in d_rw_step
    void reward_mlp_rows(const RewMlpRowsArgs& rows);
    void traj_mlp_reward_mlp(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out);
    // learned terminal value (bbmpc_set_terminal_value_mlp; bbmpc_mlp.hip, kernels_reward_mlp.hpp): a
    // network V over the state alone.  While one is installed every rollout of the handle records the trajectory and
    // k_value_mlp_terminal adds terminal_weight * V(s_H) to the scores; control steps take one launch sequence per
    // iteration (no skipped k_dist_init, no graph replay), as user_path() handles do.  One-step calls, the record and
    // bbmpc_predict_trajectories never read it.
    bool val_mlp_ready = false;
    RewMlpDesc val_mlp;
    float val_weight = 1.0f;
    DevBuf<float> d_vl_wp4[MLP_MAX_LAYERS], d_vl_bp[MLP_MAX_LAYERS], d_vl_last, d_vl_stats;
    bool value_on() const { return val_mlp_ready; }
    void set_terminal_value_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                                int is_normalized, const float* const* stats, float terminal_weight);
    void rollout_terminal_value(int mode, bool pen, RolloutArgs& ra);
    void terminal_value_rows(const float* d_states, int batch, float* d_out);
    // discounted, termination-aware returns (bbmpc_set_return_shaping; bbmpc_mlp.hip, kernels_return_shaping.hpp, DESIGN.md
    // section 8q).  While it is on every rollout of the handle records the trajectory and ends in k_shaped_return, which
    // walks each candidate's steps with the discount and the state box; a value network then enters through
    // k_reward_mlp_rows on the last plane, not through k_value_mlp_terminal.  Routed as value_on() handles are: one launch
    // sequence per iteration.  One-step calls, the record and bbmpc_predict_trajectories never read it.
    bool sh_on = false;
    float sh_gamma = 1.0f, sh_term_reward = 0.0f;
    DevBuf<float> d_sh_box, d_sh_vterm;                 // [2][S] lo | hi; [A][Nst] V of the last plane
    DevBuf<int> d_sh_tsteps;                            // [A][Nst] of the most recent rollout ...
    int sh_last_npop = 0, sh_last_Nst = 0;              // ... and its shape (0: nothing rolled out since shaping was set)
    bool shaping_on() const { return sh_on; }
    void set_return_shaping(float discount, const float* state_lo, const float* state_hi, float terminal_reward);
    void rollout_shaped(int mode, bool pen, RolloutArgs& ra);
    void termination_steps(int32_t* out, int n);
    // plan gradients (bbmpc_plan_gradient; bbmpc_mlp.hip, kernels_plan_grad.hpp): dR/da through the
    // three networks.  The setters keep the raw weights on the host (nothing else of them changes); the first gradient call
    // after a (re)install packs W and W^T of every layer with mlp_pack_layer into buffers of the feature's own.
    struct PgHostNet {
        int L = 0;
        std::vector<int> dims, acts;
        std::vector<std::vector<float>> w, b;
        void keep(int n_layers, const int32_t* d, const int32_t* a, const float* const* ws, const float* const* bs) {
            L = n_layers;
            dims.assign(d, d + n_layers + 1);
            acts.assign(a, a + n_layers);
            w.clear(); b.clear();
            for (int l = 0; l < n_layers; ++l) {
                w.emplace_back(ws[l], ws[l] + (size_t)d[l] * d[l + 1]);
                b.emplace_back(bs[l], bs[l] + d[l + 1]);
            }
        }
    };
    PgHostNet pg_host[3];              // 0 dynamics, 1 reward, 2 terminal value
    bool pg_stale[3] = {true, true, true};
    PgNet pg_net[3];
    DevBuf<float> d_pg_wf[3][MLP_MAX_LAYERS], d_pg_bf[3][MLP_MAX_LAYERS], d_pg_wr[3][MLP_MAX_LAYERS], d_pg_zero, d_pg_ws;
    void plan_gradient_check(int batch, int horizon, PlanGradArgs& q, size_t& lds, size_t& ws_floats);
    void plan_gradient_pack(int which);
    void plan_gradient_dev(const float* d_states, const float* d_seq, int batch, int horizon, float* d_returns, float* d_grad);
    void plan_gradient_eligible() const;                // the handle-level refusals of a gradient call (BBMPC_E_UNSUPPORTED)
    void plan_gradient_sizes(int batch, int horizon, PlanGradArgs& q, size_t& lds, size_t& ws_floats);   // state, arguments, sizes
    // plan refinement on the device (bbmpc_refine_plans; bbmpc_mlp.hip, kernels_plan_refine.hpp): the
    // loop gradient -> Adam / SGD step -> clip (-> keep-best) on the handle's stream, nothing in between visits the host.
    // d_rf: gradient | m | v | best [4][n rounded up to 4] | returns [B] | best returns [B]
    DevBuf<float> d_rf;
    void plan_gradient_prepare(size_t ws_floats);
    void plan_gradient_launch(PlanGradArgs q, size_t lds, const float* d_states, const float* d_seq, float* d_returns, float* d_grad);
    void refine_plans_check(int batch, int horizon, int steps, float lr, int method, int keep_best, PlanGradArgs& q, size_t& lds, size_t& wsn);
    void refine_plans_run(const PlanGradArgs& q, size_t lds, size_t wsn, const float* d_states, float* d_seq, int steps, float lr, int method,
                          int keep_best, float* d_returns_out);
    void refine_plans_dev(const float* d_states, float* d_seq, int batch, int horizon, int steps, float lr, int method, int keep_best,
                          float* d_returns_out);
    // gradient steps on CEM's candidates (bbmpc_set_grad_refine): between the elite injection and the
    // SRC_BUF rollout, columns [N - M, N) of every agent go through refine_plans_dev (keep_best = 0) from that agent's
    // state.  While it is on, control steps are routed as with elite carry (one launch sequence per iteration).
    int gr_steps = 0, gr_method = 0, gr_M = 0;          // gr_M = 0: all N columns
    float gr_lr = 0.0f;
    DevBuf<float> d_gr_rows, d_gr_states;               // [A * M][HU] | [A * M][S]
    bool grad_on() const { return gr_steps > 0; }
    void set_grad_refine(int steps, float lr, int method, int candidates);
    void grad_refine_candidates(RolloutArgs& ra);
    void set_user_source(int kind, const char* src, int nparams = 0);
    void set_user_callback(int kind, bbmpc_rows_callback fn, void* user);
    // runtime parameters of a parameterised user reward / dynamics (bbmpc_set_user_params): [A][P] on the device -- a
    // shared row is stored once per agent, so every kernel reads the row of its own agent
    struct UserParams {
        bool set = false, per_agent = false;
        DevBuf<float> d;
    };
    UserParams rew_params, dyn_params;
    int64_t rtc_compiles = 0;          // hiprtc compilations of this handle (bbmpc_compile_stats)
    void set_user_params(int kind, const float* data, int64_t count);
    const float* user_params_dev(int kind);
    const float* user_reward_params_dev();      // user_params_dev(USER_KIND_REWARD), for the units that do not see rtc.hpp
    int rows_per_agent(int kind, int batch);
    UserFunction& user_fn(int kind);            // the reward / dynamics side: its function, its parameters, ...
    UserParams& user_pp(int kind);
    void require_user_side(int kind) const;     // ... and the handle created for a user function on that side
    UserProgram user_program() const;           // what the handle's programs are compiled from (rtc.hpp)
    void launch_rows(hipFunction_t fn, int batch, void** args);
    void draw_candidates(int mode, RolloutArgs& ra);
    const float* dense_actions(const float* d_actions, int astride, int batch);
    bool user_callbacks() const { return user_reward.cb != nullptr || user_dynamics.cb != nullptr; }
    DevBuf<float> u_cb_rew;            // rewards of one planning step as a callback wrote them
    void rollout_stepwise(int mode, bool pen, RolloutArgs& ra);
    // t: the planning step a parameterised function sees (0 on one-step calls)
    void dynamics_rows(const float* d_states, const float* d_actions, int astride, int batch, float* d_next, int t = 0);
    void reward_rows(const float* d_cur, const float* d_next, const float* d_actions, int astride, int batch, float* d_total, int accumulate,
                     int t = 0);
    void mlp_forward_rows(const float* d_x, int batch, float* d_out);
    // population sharding (PI2): per-iteration partials of this rank and the gathered partials of all ranks
    DevBuf<float> ps_part, ps_all;
    DevBuf<int> c_eidx_glob;                  // sharded CMA-ES: global particle indices of the merged elites (parity trace)
    int auto_split = 0;      // > 1: population_size > 32768 is played as this many loopback shards (bbmpc.hip, constructor)
    int ps_loopback = 0;     // BBMPC_POPSHARD_LOOPBACK=G: one handle plays all G shards in turn (single-GPU test / measurement hook)
    bool ps_force = false;   // BBMPC_POPSHARD_FORCE: take the sharded code path (incl. the collective) even with one shard
    bool pop_sharded() const { return cfg.population_global > N || ps_loopback > 1 || ps_force; }
    // ... and over RANKS (the per-iteration exchange goes through the communicator): not the one-GPU splits
    bool pop_sharded_across_ranks() const { return ps_force || (ps_loopback <= 1 && cfg.population_global > N); }
    // The per-iteration exchange of a sharded population, the same for every optimizer: each shard's pass leaves a payload
    // of pw floats, all payloads meet in ps_all in shard order, the optimizer's own merge kernel reads them there.
    int shard_count() const { return ps_loopback > 1 ? ps_loopback : std::max(1, rc.comm ? rc.nranks : 1); }
    void shard_buffers(size_t pw) {
        if (!ps_part.p || ps_part.n < pw) ps_part.alloc(pw);
        if (ps_all.n < pw * shard_count()) ps_all.alloc(pw * shard_count());
    }
    // pass(population offset, destination) runs this handle's share: once into ps_part, or -- the loopback hook, a test /
    // measurement aid and the way one GPU plays a population too large for one shard -- every shard in turn, shard r =
    // particles [r*N, (r+1)*N), straight into its slot of ps_all.  pop_offset is the field of the caller's launch arguments
    // that the draws are keyed by: it follows the shard being played and is cfg.population_offset again afterwards.
    template <class Offset, class Pass>
    void play_shards(size_t pw, Offset& pop_offset, Pass&& pass) {
        if (ps_loopback > 1) {
            for (int r = 0; r < ps_loopback; ++r) {
                pop_offset = r * N;
                pass(r * N, ps_all.p + pw * r);
            }
            pop_offset = cfg.population_offset;
        } else {
            pass((int)cfg.population_offset, ps_part.p);
        }
    }
    void gather_shards(size_t pw, const char* what);     // ps_part of every rank -> ps_all (nothing to do under the loopback hook)
    // CMA-ES at n <= 32 on the analytic pendulum: the last iteration's update launch is held back until finalize() knows the
    // record's arguments and then carries the tail of the control step as well (kernels_eigh_small.hpp)
    struct PendingCmaUpdate { bool set = false; CmaArgs q; size_t lds = 0; int yef = 0; } pending_cma_update;
    int pending_warm = 0;    // learned-dynamics path: warm start the tail kernel performs (kernels_tail.hpp TailArgs::warm_mode)
    RowMlp row_mlp() const;
    bool any_injected() const {
        for (const auto& kv : inj) if (kv.second.p) return true;
        return false;
    }
    const float* injected(int kind) const {
        auto it = inj.find(kind);
        return (it == inj.end() || !it->second.p) ? nullptr : it->second.p;
    }
    float* pinned(size_t count);

    void reset();
    void optimize_dev(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out);
    void launch_pending_cma_update(const FinalArgs& fa);
    bool use_fused_pso() const;
    void optimize_fused_pso(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out, uint32_t step);
    bool use_fused_cma() const;
    void optimize_fused_cma(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out, uint32_t step);
    bool use_fused() const;
    void optimize_fused(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out, uint32_t step);
    void ensure_trace();
    RefitArgs refit_args() const;
    // CEM / PI2 on the learned model: what both ask before a control step opens without k_dist_init, and the first rollout
    // of a control step (bbmpc.hip)
    bool dist_init_skippable() const;
    bool first_rollout_mlp(bool pen, RolloutArgs& ra, const float* mean, const float* sigma, const float* pinned_state);
    void optimize_random_search(RolloutArgs& ra);
    void optimize_cem(RolloutArgs& ra);
    void optimize_pi2(RolloutArgs& ra);
    void optimize_spsa(RolloutArgs& ra, uint32_t step);
    void optimize_pso(RolloutArgs& ra, uint32_t step);
    void optimize_cma(RolloutArgs& ra, uint32_t step);
    void cma_init();
    void cma_reset_mean_sigma();
    CmaArgs cma_args(uint32_t step, uint32_t iter);
    OptArgs opt_args(uint32_t step, uint32_t iter) const;
    PsoState pso_state(int shard = 0);       // shard > 0: the loopback hook's further copies of the per-particle state
    void evaluate_dev(const float* d_state_in, const float* d_seq, int n_pop, float* d_rew_out);
    void step_dev(const float* d_states, const float* d_actions, int astride, int batch, float* d_next, float* d_rew);
    void reward_dev(const float* d_cur, const float* d_next, const float* d_act, int batch, float* d_rew);
    // open-loop trajectory prediction (bbmpc_traj.hip; the learned model's MFMA kernel is launched from bbmpc_mlp.hip):
    // states [B,S], sequences [B,Hq,U] -> states_out [B,Hq,S], rewards_out [B,Hq] (either may be null)
    void predict_trajectories_dev(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out);
    void traj_mlp(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out);
    void traj_user_fused(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out);   // bbmpc_user.hip
    UserFunction user_traj;            // rtc.hpp bbmpc_user_traj, built on the first prediction
    bool user_traj_stale = true;
    // plan readback (bbmpc_set_keep_plan / bbmpc_get_plan): the switch routes control steps as bbmpc_set_trace does, so the
    // solution of every iteration stays in HBM
    bool keep_plan = false;
    bool plan_ready = false;           // a control step ran since the switch went on
    void get_plan(float* actions_out);
    // particle trajectory evaluator (bbmpc_set_particles; bbmpc_particles.hip, kernels_particles.hpp): P noisy rollouts per
    // candidate reduced to mean - kappa * std.  While it is on, control steps are routed as bbmpc_set_trace routes them
    // (one launch sequence per iteration: no resident, fused or graph-replayed form) and launch_rollout scores through it.
    int part_P = 0;
    float part_kappa = 0.0f;
    // how the P returns become the score (bbmpc_set_particle_risk): mean - kappa * std, or the mean of
    // the part_tail worst returns (CVaR; kappa is then ignored).  Kept while particles are off.
    int part_risk = BBMPC_RISK_MEAN_STD, part_tail = 0;
    void set_particle_risk(int kind, int tail_count);
    DevBuf<float> d_psigma, d_pnoise, d_preturns;   // sigma [S] | eps [A][P][H][S] | returns [A][Nst * P]
    bool pnoise_valid = false;         // d_pnoise holds the draws of (pnoise_step, pnoise_iter)
    uint32_t pnoise_step = 0, pnoise_iter = 0;
    bool particles_on() const { return part_P > 0; }
    void set_particles(int num_particles, const float* sigma, float kappa);
    const float* process_noise(uint32_t step, uint32_t iter);
    void dump_process_noise(int control_step, int iteration, float* out, int64_t count);
    void rollout_particles(int mode, bool pen, RolloutArgs& ra, float* d_returns, int returns_stride);
    void launch_rollout_mlp_particles(const ParticleArgs& pa);                 // bbmpc_mlp.hip
    // a HIP-source reward over the learned model's particles: the rollout stores every noisy next state
    // to d_ptraj [H][A][S][RS] (ParticleArgs::traj), rtc.hpp's scorers turn states into returns / per-step rewards
    DevBuf<float> d_ptraj;
    bool particle_user_reward() const { return cfg.dynamics == BBMPC_DYN_MLP && cfg.reward == BBMPC_REW_USER && !has_xform(); }
    void require_particle_user_reward() const;                                // bbmpc_user.hip: what this path refuses at compute time
    void score_particles_user(const ParticleArgs& pa);                        // bbmpc_particles.hip
    void require_particle_traj_fits(long returns_stride) const;               // H * A * S * RS < 2^31, before anything is allocated
    void score_traj_particles_user(const TrajParticleArgs& pa);               // bbmpc_user.hip
    // chance constraint (bbmpc_set_chance_constraint; bbmpc_particles.hip, kernels_particle_constraint.hpp, DESIGN.md section
    // 8t): a state box over the noisy states of the learned model's particle rollouts.  While it is installed the rollout
    // takes the TRAJ form whatever the reward, k_particle_box_scan finds every row's first step outside the box (and, for a
    // built-in reward, the row's return) and k_particle_constraint_apply subtracts weight * max(0, v - max_violation) from
    // the aggregate's score.  Removed by bbmpc_set_particles(0).
    bool cc_on = false;
    float cc_delta = 0.0f, cc_lambda = 0.0f;
    DevBuf<float> d_cc_box, d_cc_viol;                  // [2][S] lo | hi; [A][Nst] v of the most recent rollout ...
    DevBuf<int> d_cc_first;                             // ... and its first steps [A][RS]
    int cc_last_npop = 0, cc_last_Nst = 0, cc_last_RS = 0, cc_last_P = 0;      // its shape (0: nothing rolled out since the install)
    bool constraint_on() const { return cc_on; }
    void set_chance_constraint(const float* lo, const float* hi, float max_violation, float weight);
    void constraint_violations(int n_pop, float* prob_out, int32_t* first_out);
    bool constraint_raw_state(const std::string& name, float* out, const float* in, int64_t count);   // get_state / set_state names of tests
    // model ensemble for the particle rollouts (bbmpc_set_mlp_ensemble; bbmpc_mlp.hip, kernels_mlp_particles.hpp): particle p
    // follows member p % ens_E.  Every deterministic path keeps the model of bbmpc_set_mlp.
    int ens_E = 0;
    DevBuf<float> d_ens_wp4[MLP_MAX_LAYERS], d_ens_bp[MLP_MAX_LAYERS];   // per layer [E][OT][IT][64][4] | [E][OT][64][4]
    void set_mlp_ensemble(int E, const float* const* w, const float* const* b);
    // log-variance heads of the model / of every member (bbmpc_set_mlp_logvar_head; bbmpc_mlp.hip, kernels_mlp_particles.hpp):
    // the particle rollouts add (sigma + sd(s, a)) * eps.  lv_heads = max(1, ens_E) while installed, else 0; removed by
    // bbmpc_set_mlp and bbmpc_set_mlp_ensemble.  No deterministic path reads them.
    int lv_heads = 0;
    DevBuf<float> d_lv_wp4, d_lv_bp, d_lv_bounds;                        // [heads][OT][IT][64][4] | [heads][OT][64][4] | min [S], max [S]
    void set_mlp_logvar_head(int num_heads, const float* const* w, const float* const* b, const float* min_logvar, const float* max_logvar);
    void evaluate_particles_dev(const float* d_state_in, const float* d_seq, int n_pop, float* d_scores, float* d_returns);
    // trajectory distributions (bbmpc_predict_trajectory_particles; bbmpc_traj_particles.hip, kernels_traj_particles.hpp): the
    // particle recurrence from every row's own start state, every state and reward kept, and their moments over the particles.
    // Buffers of its own: the draws [B][P][Hq][S] (never d_pnoise, whose validity flags belong to the control step), the
    // particle tensors when the caller does not want them.
    DevBuf<float> tjp_noise, tjp_ps, tjp_pr;
    void predict_trajectory_particles_dev(const float* d_states, const float* d_seq, int batch, int horizon, const float* d_eps,
                                          float* d_smean, float* d_sstd, float* d_rmean, float* d_rstd, float* d_pstates, float* d_prewards);
    void launch_traj_mlp_particles(const TrajParticleArgs& pa);               // bbmpc_mlp.hip
    // draws (unless supplied) -> noisy trajectories into d_pstates / d_prewards (null: the handle's scratch, returned)
    void roll_trajectory_particles(const float* d_states, const float* d_seq, int batch, int horizon, const float* d_eps, float*& d_pstates,
                                   float*& d_prewards);
    // the same with nearest-rank quantiles over the particles (bbmpc_predict_trajectory_quantiles)
    void predict_trajectory_quantiles_dev(const float* d_states, const float* d_seq, int batch, int horizon, const float* d_eps, float* d_smean,
                                          float* d_sstd, float* d_rmean, float* d_rstd, float* d_pstates, float* d_prewards, int num_levels,
                                          const int32_t* ranks, float* d_squant, float* d_rquant);
    // temporally correlated sampling for CEM / PI2 (bbmpc_set_sampling_correlation; kernels_corr.hpp):
    // one H x H mixing matrix applied along the time axis of the standard draws.  While it is installed, control steps are
    // routed as bbmpc_set_trace routes them (one launch sequence per iteration: no resident, fused or graph-replayed form)
    // and launch_rollout draws the candidates into the sample buffer, then rolls them out in the SRC_BUF form.
    DevBuf<float> d_corr_mix;          // [H][H] row-major
    DevBuf<int> d_corr_end;            // [H] per row: index after the last non-zero column (at least 1)
    bool corr_installed = false;
    bool corr_on() const { return corr_installed; }
    void set_sampling_correlation(const float* mix, int64_t count);
    void draw_candidates_corr(RolloutArgs& ra);
    // elite carry-over for CEM (bbmpc_set_elite_carry; kernels_elite_carry.hpp): the best carry_keep
    // elites of an iteration replace the last candidates of the next one, the best carry_shift of a control step's last
    // iteration, moved one planning step forward, those of the next control step's first iteration.  While it is on,
    // control steps are routed as with a mixing matrix (one launch sequence per iteration) and launch_rollout draws the
    // candidates into the sample buffer, overwrites its last columns, then rolls them out in the SRC_BUF form.
    int carry_keep = 0, carry_shift = 0;
    int carry_stored = 0;              // shifted elites held for the next control step (0 after reset and after the setter)
    int carry_inject = 0;              // columns the next CEM draw is followed by (set by optimize_cem around launch_rollout)
    DevBuf<float> d_carry;             // [A][HU][max(carry_keep, carry_shift)]
    bool carry_on() const { return carry_keep > 0 || carry_shift > 0; }
    int carry_stride() const { return std::max(carry_keep, carry_shift); }
    void set_elite_carry(int keep, int shift);
    void save_elites(int count, bool shift);
    // learned policy prior for CEM (bbmpc_set_policy_prior_mlp; bbmpc_mlp.hip, kernels_policy_prior.hpp, DESIGN.md section
    // 8l): prior_K closed-loop rollouts of a policy network through the learned model overwrite the candidate columns in
    // front of the carried elites, between the draw and the SRC_BUF rollout.  While it is on, control steps are routed as
    // with elite carry (one launch sequence per iteration).
    bool prior_ready = false;
    MlpDesc prior_mlp;                 // dims[0] = S, dims[L] = U; mean_s / std_s = mean_in / std_in, mean_t / std_t = mean_out / std_out
    int prior_nw = 1;                  // waves its widest hidden layer asks for
    int prior_K = 0;
    float prior_sigma = 0.0f;
    DevBuf<float> d_pr_wp4[MLP_MAX_LAYERS], d_pr_bp[MLP_MAX_LAYERS], d_pr_stats, d_pr_noise;
    bool prior_noise_valid = false;    // d_pr_noise holds the draws of (prior_noise_step, prior_noise_iter)
    uint32_t prior_noise_step = 0, prior_noise_iter = 0;
    bool prior_on() const { return prior_ready; }
    void set_policy_prior_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                              int is_normalized, const float* const* stats, int count, float noise_std);
    const float* policy_noise(uint32_t step, uint32_t iter);
    void dump_policy_noise(int control_step, int iteration, float* out, int64_t count);
    void policy_prior_rollouts(const float* d_state, const float* d_noise, float* samples, int nst, int col0, float* d_actions_out,
                               float* d_states_out);
    void policy_prior_rows(const float* d_states, int batch, float* d_actions);
    void traj_stepwise(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out);
    void traj_sq_error_dev(const float* d_pred, const float* d_obs, int batch, int horizon, double* d_sumsq);
    DevBuf<float> tj_x0, tj_x1, tj_rew;             // step-wise form: dense state ping-pong and one step's rewards
    DevBuf<double> tj_part;                          // squared-error partials [row blocks][Hq*S]

    void inject(int kind, const float* data, int64_t count);
    void dump_noise(int kind, int control_step, int iteration, float* out, int64_t count);
    void get_trace(int iteration, int item, void* out, int64_t bytes);
    void get_state(const std::string& name, float* out, int64_t count);
    void set_state(const std::string& name, const float* data, int64_t count);
    void get_profile(double* ms, int64_t* launches);

    // helpers
    void launch_rollout(int mode, bool pen, RolloutArgs& ra);
    // traj_out: [H][A][Nst][S], the state after every step (u_traj), or nullptr
    void launch_rollout_mlp(int mode, bool pen, RolloutArgs& ra, bool per_particle_state, float* final_state, float* traj_out);
    MlpLaunch choose_rollout_mlp(const RolloutArgs& ra, bool per_particle_state, bool final_state, bool record) const;   // bbmpc_mlp.hip
    void set_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                 int is_normalized, const float* const* stats);
    void prof_begin();
    void prof_end();
    void capture_trace(int it);
    void finalize(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out, uint32_t step);
    void to_internal(const float* ref, int n_pop, float* internal_host) const;     // [n,A,H,U] -> [A][HU][Nst]
    void from_internal(const float* internal_host, int n_pop, float* ref) const;
};

}  // namespace bbmpc
