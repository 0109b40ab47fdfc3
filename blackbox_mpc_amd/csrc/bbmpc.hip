// C ABI (include/bbmpc.h) + engine implementation.  gfx950 only, no CPU fallback.
#include "engine.hpp"
#include "abi_util.hpp"
#include "engine_util.hpp"
#include "kernels_corr.hpp"
#include "kernels_elite_carry.hpp"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <functional>
#include <chrono>
#include <mutex>
#include <set>
#include <thread>
#include <utility>

namespace bbmpc {

// every live handle of the process (see Engine::mbox_pub)
static std::mutex g_engines_mu;
static std::set<Engine*> g_engines;
static std::atomic<int> g_resident_handles{0};
void note_resident_handle() { g_resident_handles.fetch_add(1, std::memory_order_relaxed); }   // (bbmpc_fused.hip publishes a mailbox)

// Called at every entry point: resident workgroups of OTHER handles on this device are asked to leave (a few stores into
// pinned memory, no synchronisation); costs one relaxed load when nothing is resident.
void stop_foreign_residents(Engine* self) {
    const int mine = (self && self->mbox_pub.load(std::memory_order_relaxed)) ? 1 : 0;
    if (g_resident_handles.load(std::memory_order_relaxed) - mine <= 0) return;
    std::lock_guard<std::mutex> lock(g_engines_mu);
    for (Engine* o : g_engines) {
        if (o == self || (self && o->device != self->device)) continue;
        uint32_t* m = o->mbox_pub.load(std::memory_order_acquire);
        if (!m) continue;
        for (int a = 0; a < o->mbox_pub_agents; ++a) ((volatile uint32_t*)m)[a * 16 + 15] = 0xffffffffu;   // the stop word
        std::atomic_thread_fence(std::memory_order_release);
    }
}

thread_local std::string g_last_error;     // (abi_util.hpp)

// ------------------------------------------------------------------------------------------------
// construction
// ------------------------------------------------------------------------------------------------
// truncated-normal quantile table (rng.hpp): q(i/2048) in float64 -> fp32, uploaded once per device
static double erfinv_d(double y) {
    // Newton on erf from a Giles-type start; converges to double precision in a few steps for |y| < 0.96
    double w = -log((1.0 - y) * (1.0 + y)), x;
    if (w < 5.0) {
        w -= 2.5;
        x = 2.81022636e-08; x = 3.43273939e-07 + x * w; x = -3.5233877e-06 + x * w; x = -4.39150654e-06 + x * w;
        x = 0.00021858087 + x * w; x = -0.00125372503 + x * w; x = -0.00417768164 + x * w; x = 0.246640727 + x * w;
        x = 1.50140941 + x * w;
    } else {
        w = sqrt(w) - 3.0;
        x = -0.000200214257; x = 0.000100950558 + x * w; x = 0.00134934322 + x * w; x = -0.00367342844 + x * w;
        x = 0.00573950773 + x * w; x = -0.0076224613 + x * w; x = 0.00943887047 + x * w; x = 1.00167406 + x * w;
        x = 2.83297682 + x * w;
    }
    x *= y;
    for (int it = 0; it < 4; ++it) x -= (erf(x) - y) / (1.1283791670955126 * exp(-x * x));
    return x;
}

static void init_tnq_table() {
    // per-device symbol, uploaded once; handles may be created from several threads (a thread-per-GPU driver)
    static std::mutex mu;
    static std::set<int> done;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (done.count(dev)) return;
    std::vector<float> q(TNQ_SIZE + 1);
    const double p2 = erf(sqrt(2.0));                       // P(|z| < 2)
    for (int i = 0; i <= TNQ_SIZE; ++i) q[i] = (float)(sqrt(2.0) * erfinv_d((2.0 * i / TNQ_SIZE - 1.0) * p2));
    q[0] = -2.0f;
    q[TNQ_SIZE] = 2.0f;
    std::vector<float2> tab(TNQ_SIZE);
    for (int i = 0; i < TNQ_SIZE; ++i) tab[i] = make_float2(q[i], q[i + 1] - q[i]);
    tnq_upload(tab.data());                                  // this translation unit's copy ...
    bbmpc_tu_cma_upload_tnq(tab.data());                     // ... and the other two
    bbmpc_tu_mlp_upload_tnq(tab.data());
    bbmpc_tu_fused_upload_tnq(tab.data());
    done.insert(dev);                                       // only after the upload succeeded
}

// "lo-hi" in the environment variable `name` -> a stream whose workgroups only go to CUs lo .. hi (hipExtStreamCreateWithCUMask,
// bit i of the mask = CU i), or null when the variable is not set
hipStream_t masked_stream_from_env(const char* name, int cu_count) {
    const char* v = getenv(name);
    int lo = 0, hi = 0;
    if (!v || sscanf(v, "%d-%d", &lo, &hi) != 2 || lo < 0 || hi < lo || hi >= cu_count) return nullptr;
    std::vector<uint32_t> mask((size_t)(cu_count + 31) / 32, 0u);
    for (int c = lo; c <= hi; ++c) mask[(size_t)c >> 5] |= 1u << (c & 31);
    hipStream_t st = nullptr;
    HIP_CHECK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
    return st;
}

Engine::Engine(const bbmpc_config& c) : cfg(c) {
    REQUIRE(c.abi_version == BBMPC_ABI_VERSION, BBMPC_E_INVALID, "bbmpc_config.abi_version mismatch");
    stop_foreign_residents(nullptr);     // creation allocates and copies: nothing should wait behind a lingering kernel
    N = c.population_size; A = c.num_agents; H = c.planning_horizon; U = c.dim_u; S = c.dim_s;
    iters = c.optimizer == BBMPC_OPT_RANDOM_SEARCH ? 1 : c.max_iterations;
    if (c.optimizer == BBMPC_OPT_NONE) iters = 0;
    k = c.num_elite;
    REQUIRE(A >= 1 && H >= 1 && U >= 1 && S >= 1, BBMPC_E_INVALID, "num_agents, planning_horizon, dim_u, dim_s must be >= 1");
    REQUIRE(c.action_low && c.action_high, BBMPC_E_INVALID, "action_low/action_high are required");
    REQUIRE(c.optimizer >= BBMPC_OPT_NONE && c.optimizer <= BBMPC_OPT_SPSA, BBMPC_E_INVALID, "unknown optimizer");
    REQUIRE(c.dynamics == BBMPC_DYN_PENDULUM || c.dynamics == BBMPC_DYN_MLP || c.dynamics == BBMPC_DYN_USER, BBMPC_E_INVALID, "unknown dynamics kind");
    REQUIRE(c.reward == BBMPC_REW_PENDULUM || c.reward == BBMPC_REW_CHEETAH || c.reward == BBMPC_REW_USER || c.reward == BBMPC_REW_MLP,
            BBMPC_E_INVALID, "unknown reward kind");
    if (c.reward == BBMPC_REW_MLP)
        REQUIRE(c.dynamics == BBMPC_DYN_MLP, BBMPC_E_UNSUPPORTED,
                "a learned reward model (BBMPC_REW_MLP) scores the rollouts of a learned model: the handle needs BBMPC_DYN_MLP, not analytic or user dynamics");
    if (c.dynamics == BBMPC_DYN_USER || c.reward == BBMPC_REW_USER)
        REQUIRE(S <= 256 && U <= 256, BBMPC_E_UNSUPPORTED, "user device functions: dim_s, dim_u <= 256 (per-row arrays live in registers)");
    if (c.dynamics == BBMPC_DYN_PENDULUM)
        REQUIRE(S == 3 && U == 1, BBMPC_E_INVALID, "PendulumTrueModel needs dim_s == 3 and dim_u == 1");
    if (c.reward == BBMPC_REW_PENDULUM) REQUIRE(S >= 3, BBMPC_E_INVALID, "pendulum reward needs dim_s >= 3");
    if (c.reward == BBMPC_REW_CHEETAH) REQUIRE(S >= 18, BBMPC_E_INVALID, "cheetah reward indexes state[17]: dim_s >= 18");
    if (c.optimizer != BBMPC_OPT_NONE) {
        REQUIRE(N >= 1, BBMPC_E_INVALID, "population_size must be >= 1");
        REQUIRE(iters >= 0, BBMPC_E_INVALID, "max_iterations must be >= 0");
        if (N > 32768) {
            // The refit kernels keep an agent's rewards in one CU's LDS (32768 floats).  A larger population is played as G
            // equal shards of the population-sharding machinery on this one GPU: shard r = particles
            // [r N/G, (r+1) N/G), draws keyed by the global particle, one merge per iteration -- the loopback hook, switched on
            // by the size.  The parity hooks (trace, injected noise, per-particle state) stay per shard and are refused.
            REQUIRE(c.population_global == 0 && c.population_offset == 0, BBMPC_E_UNSUPPORTED,
                    "population_size > 32768 per rank: give every rank at most 32768 particles of the sharded population");
            int g = (N + 32767) / 32768;
            while (g <= 64 && N % g != 0) ++g;
            REQUIRE(g <= 64, BBMPC_E_UNSUPPORTED, "population_size > 32768 must divide into at most 64 equal shards of at most 32768 particles");
            if (c.optimizer == BBMPC_OPT_CMAES) REQUIRE(k <= N / g, BBMPC_E_UNSUPPORTED, "num_elite must not exceed a shard of the population");
            auto_split = g;
            cfg.population_global = N;
            N /= g;
        }
    } else {
        N = 0;
    }
    if (c.optimizer == BBMPC_OPT_CEM || c.optimizer == BBMPC_OPT_CMAES)
        REQUIRE(k >= 1 && k <= std::max(N, (int)c.population_global), BBMPC_E_INVALID, "num_elite must be in [1, population_size]");
    if (c.optimizer == BBMPC_OPT_CEM) REQUIRE(k <= 1024, BBMPC_E_UNSUPPORTED, "num_elite > 1024 not supported");
    if (c.optimizer == BBMPC_OPT_CMAES) {
        const bool per_agent = (c.quirks & BBMPC_CMAES_PER_AGENT) != 0;
        const long nn = per_agent ? (long)H * U : (long)A * H * U;
        REQUIRE(nn <= 4096, BBMPC_E_UNSUPPORTED,
                "CMA-ES joint dimension num_agents*H*U > 4096: use BBMPC_CMAES_PER_AGENT (the reference's own "
                "[N,n,n] map_fn stack cannot run at this size either, cma_es.py:13)");
        REQUIRE(per_agent || c.num_agents_global <= c.num_agents, BBMPC_E_UNSUPPORTED,
                "coupled CMA-ES sums rewards over ALL agents and does not shard; use BBMPC_CMAES_PER_AGENT");
        REQUIRE(k <= 1024, BBMPC_E_UNSUPPORTED, "num_elite > 1024 not supported");
    }

    if (c.population_global != 0 || c.population_offset != 0) {
        REQUIRE(c.population_global >= N && c.population_offset >= 0 && c.population_offset + N <= c.population_global, BBMPC_E_INVALID,
                "population_offset / population_global: this handle's particles must lie inside the global population");
        if (c.population_global > N) {
            REQUIRE(c.optimizer != BBMPC_OPT_NONE, BBMPC_E_UNSUPPORTED, "population sharding needs an optimizer (evaluate-only handles roll out what they are given)");
            if (c.optimizer == BBMPC_OPT_CMAES)
                REQUIRE(k <= N && k <= 1024, BBMPC_E_UNSUPPORTED, "sharded CMA-ES: num_elite must not exceed this rank's share of the population (nor 1024)");
        }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw HipError(BBMPC_E_NO_DEVICE, "no HIP device available: this library has no CPU fallback");
    if (c.device >= 0) {
        REQUIRE(c.device < ndev, BBMPC_E_NO_DEVICE, "bbmpc_config.device out of range");
        HIP_CHECK(hipSetDevice(c.device));        // bbmpc_create restores the caller's device (DeviceGuard)
    }
    HIP_CHECK(hipGetDevice(&device));
    HIP_CHECK(hipDeviceGetAttribute(&cu_count, hipDeviceAttributeMultiprocessorCount, device));
    {   // control steps are latency-critical, and a resident control-step kernel must not hold back unrelated work of the
        // process: hardware queues are pooled per priority, so the handle's streams live in the high-priority pool, away
        // from PyTorch's and the caller's normal-priority streams (the handles among themselves: stop_foreign_residents)
        int least = 0, greatest = 0;
        HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
        // experiment switch (profiles/r5_cfg5cma_overlap.md): BBMPC_STREAM_CUS=lo-hi confines the handle's stream to those CUs
        if (!(own_stream = masked_stream_from_env("BBMPC_STREAM_CUS", cu_count)))
            HIP_CHECK(hipStreamCreateWithPriority(&own_stream, hipStreamNonBlocking, greatest));
    }
    stream = own_stream;
    init_tnq_table();

    if (const char* fm = getenv("BBMPC_FUSED")) fused_mode = atoi(fm);
    {
        auto flag = [](const char* n) { return getenv(n) != nullptr; };
        auto ival = [](const char* n, int dflt) { const char* v = getenv(n); return v ? atoi(v) : dflt; };
        sw.cma_svd_v1 = flag("BBMPC_CMA_SVD_V1"); sw.cma_svd_rounds = flag("BBMPC_CMA_SVD_ROUNDS");
        sw.cma_svd_general = flag("BBMPC_CMA_SVD_GENERAL");
        sw.cma_svd_gram = flag("BBMPC_CMA_SVD_GRAM");
        sw.cma_coop = flag("BBMPC_CMA_COOP"); sw.cma_nb = ival("BBMPC_CMA_NB", 0);
        sw.cma_eigh = ival("BBMPC_CMA_EIGH", 1); sw.cma_eigh_fail = flag("BBMPC_CMA_EIGH_FAIL");
        sw.cma_fused = flag("BBMPC_CMA_FUSED");
        sw.mlp_generic = flag("BBMPC_MLP_GENERIC");
        { const int b = ival("BBMPC_MLP_BF16", 0); sw.mlp_bf16 = (b == 1 || b == 3) ? b : 0; }
        sw.mlp_pair = ival("BBMPC_MLP_PAIR", -1); sw.mlp_q4 = ival("BBMPC_MLP_Q4", -1); sw.mlp_q4s = ival("BBMPC_MLP_Q4S", ival("BBMPC_MLP_Q4R", 1)); sw.mlp_w4 = ival("BBMPC_MLP_W4", 1); sw.pi2_skip_init = ival("BBMPC_PI2_SKIP_INIT", 1); sw.step_graph = ival("BBMPC_STEP_GRAPH", 1); sw.cma_small3 = ival("BBMPC_CMA_SMALL3", 1);
        sw.refit_wgs = ival("BBMPC_REFIT_WGS", 0);
        sw.mlp_wave = ival("BBMPC_MLP_WAVE", 1);
        sw.linger_us = std::max(0, ival("BBMPC_LINGER_US", 200));
        if (const char* fb = getenv("BBMPC_FUSED_BOUND")) {
            sw.fused_bound = atoi(fb);
            REQUIRE(sw.fused_bound == 512 || sw.fused_bound == 1024, BBMPC_E_INVALID, "BBMPC_FUSED_BOUND must be 512, 1024 or unset");
        }
        sw.cem_wave_select = ival("BBMPC_CEM_WAVE_SELECT", 1) != 0 ? 1 : 0;
        sw.trace_select_only = flag("BBMPC_TRACE_SELECT_ONLY");
        linger_test_quit = ival("BBMPC_LINGER_TEST_QUIT", 0) - 1;
        host_seq = (uint32_t)ival("BBMPC_TEST_HOST_SEQ", 0);      // test hook: where the completion sequence numbers start (the 16-bit tag's wrap)
        sw.balance = ival("BBMPC_BALANCE", 0);      // accepted and ignored: pacing SIMD mates in the fused pendulum rollout measured slower and is gone
        sw.ilp = ival("BBMPC_ILP", 1) == 2 ? 2 : 1;
        sw.refit_v1 = flag("BBMPC_REFIT_V1");
        sw.zero_copy = !flag("BBMPC_NO_ZERO_COPY");
        sw.host_poll = !flag("BBMPC_NO_HOST_POLL");
        sw.mlp_no_half_tail = flag("BBMPC_MLP_NO_HALF_TAIL");
        sw.dbg = flag("BBMPC_DBG");
        sw.prof_reward_mlp = flag("BBMPC_PROF_REWARD_MLP");
        user_stepwise_only = flag("BBMPC_USER_STEPWISE");
        if (c.optimizer != BBMPC_OPT_NONE) {
            ps_loopback = auto_split > 1 ? auto_split : ival("BBMPC_POPSHARD_LOOPBACK", 0);
            ps_force = flag("BBMPC_POPSHARD_FORCE");
        }
    }
    HU = H * U;
    Nst = ((std::max(N, 1) + 63) / 64) * 64;
    rec = U + S + 1;
    lo.assign(c.action_low, c.action_low + U);
    hi.assign(c.action_high, c.action_high + U);
    upload(d_lo, lo);
    upload(d_hi, hi);
    d_state.alloc((size_t)A * S);
    d_record.alloc((size_t)A * rec);
    d_action.alloc((size_t)A * U);
    d_action.zero(stream);
    if (c.optimizer != BBMPC_OPT_NONE) {
        // mean = (lo+hi)/2, var = (lo-hi)^2/16 tiled to [A,H,U]   cem.py:55-72, pi2.py:44-55
        std::vector<float> m((size_t)A * HU), v((size_t)A * HU);
        for (int i = 0; i < A * HU; ++i) {
            const int u = i % U;
            m[i] = (lo[u] + hi[u]) / 2.0f;
            const float d = lo[u] - hi[u];
            v[i] = (d * d) / 16.0f;
        }
        upload(d_prev_mean, m);
        upload(d_var0, v);
        d_mean.alloc(m.size());
        d_var.alloc(m.size());
        d_sigma.alloc(m.size());
        d_samples.alloc((size_t)A * HU * Nst);
        d_rewards.alloc((size_t)A * Nst);
        d_penalty.alloc((size_t)A * Nst);
        d_elites.alloc((size_t)A * std::max(k, 1));
        const size_t big = (size_t)A * HU * Nst;
        if (c.optimizer == BBMPC_OPT_SPSA) {
            d_cand_a.alloc(big);
            d_cand_b.alloc(big);
            d_rewards2.alloc((size_t)A * Nst);
        }
        if (c.optimizer == BBMPC_OPT_CMAES) {
            d_cand_a.alloc(big);
            cma_init();
        }
        if (c.optimizer == BBMPC_OPT_PSO) {
            // constructor state of the reference: every Variable zero (pso.py:50-59), quirk Q4
            const size_t gl = ps_loopback > 1 ? (size_t)ps_loopback : 1;      // the loopback hook keeps every shard's swarm
            d_cand_a.alloc(big * gl); d_vel.alloc(big * gl); d_pbest.alloc(big * gl);
            d_pbest_r.alloc((size_t)A * Nst * gl); d_cond.alloc((size_t)A * Nst * gl);
            d_gbest.alloc((size_t)A * HU); d_gbest_r.alloc((size_t)A); d_gidx.alloc((size_t)A);
            d_cand_a.zero(stream); d_vel.zero(stream); d_pbest.zero(stream); d_pbest_r.zero(stream);
            d_cond.zero(stream); d_gbest.zero(stream); d_gbest_r.zero(stream); d_gidx.zero(stream);
        }
    }
    HIP_CHECK(hipStreamSynchronize(stream));
    // registered last: a constructor that throws never runs the destructor
    { std::lock_guard<std::mutex> lock(g_engines_mu); g_engines.insert(this); }
}

Engine::~Engine() {
    try { resident_stop(); } catch (...) {}
    if (step_graph) { (void)hipGraphExecDestroy(step_graph); step_graph = nullptr; }
    if (step_words) { (void)hipHostFree(step_words); step_words = nullptr; }
    if (step_words_dev) { (void)hipFree(step_words_dev); step_words_dev = nullptr; }
    { std::lock_guard<std::mutex> lock(g_engines_mu); g_engines.erase(this); }
    if (lazy_sync && stream) (void)hipStreamSynchronize(stream);
    if (own_stream) (void)hipStreamSynchronize(own_stream);
    rc.destroy();
    if (eigh_side) {
        (void)hipStreamSynchronize(eigh_side);
        (void)hipStreamDestroy(eigh_side);
        for (int i = 0; i < 2; ++i) if (eigh_ev[i]) (void)hipEventDestroy(eigh_ev[i]);
    }
    if (pf_stream) {
        (void)hipStreamSynchronize(pf_stream);
        (void)hipStreamDestroy(pf_stream);
        for (int b = 0; b < 2; ++b)
            if (pf_done[b]) (void)hipEventDestroy(pf_done[b]);
        if (pf_free) (void)hipEventDestroy(pf_free);
    }
    for (auto e : ev_pool) (void)hipEventDestroy(e);
    user_reward.release();
    user_dynamics.release();
    user_rollout.release();
    user_xform.release();
    user_fwd_xform.release();
    user_xform_rollout.release();
    if (h_pin) (void)hipHostFree(h_pin);
    for (auto*& hs : h_record_stage) { if (hs) (void)hipHostFree(hs); hs = nullptr; }
    if (host_done) (void)hipHostFree(host_done);
    if (host_count) (void)hipFree(host_count);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

void Engine::settle() {
    if (settle_hook) settle_hook(this);          // staged records of bbmpc_optimize_gather go to the collective first
    resident_stop();
    if (lazy_sync) {
        lazy_sync = false;
        HIP_CHECK(hipStreamSynchronize(stream));
    }
}

static void resident_unpublish(Engine* e);

// The resident workgroups' side of this is at the end of k_fused_pendulum.  Returns false when the call has to go through
// a launch after all: the workgroups left (the stream is idle then), this step's noise chunk is not there yet, or -- a
// request that crossed some workgroups' exit -- only part of the agents were served: subset_n / amap_host() then name the
// rest and the launch that follows covers exactly those.
bool Engine::resident_step(const float* state, int add_noise, uint32_t seq, float* records) {
    {   // all workgroups gone already (linger time over, or another handle asked them to leave): nothing to stop or wait for
        bool all_gone = true;
        for (int a = 0; a < A && all_gone; ++a) all_gone = *(volatile const uint32_t*)gone_host(a) != 0u;
        if (all_gone) {
            resident_unpublish(this);
            resident_alive = false;
            return false;
        }
    }
    const uint32_t step = step_counter;
    const int64_t c = (int64_t)step / std::max(pf_steps, 1);
    const int pb = (int)(c & 1), nb = pb ^ 1;
    if (pf_mode != 1 || pf_chunk[pb] != c) { resident_stop(); return false; }
    if (!pf_waited[pb]) {
        if (hipEventQuery(pf_done[pb]) != hipSuccess) { resident_stop(); return false; }
        pf_waited[pb] = true; pf_inflight[pb] = false;
    }
    const float* inj = d_noise_pf[pb].p + (size_t)((int64_t)step - c * pf_steps) * pf_step_floats;
    ++step_counter;
    const uint64_t ip = (uint64_t)(uintptr_t)inj;
    // One request line per agent.  Every payload word carries 16 bits of payload and the low 16 bits of the request's
    // sequence number, word 15 the whole sequence number: the kernel accepts a line only when all fourteen words name
    // the request it waits for, so nothing depends on the 64-byte line being read (or written) in one piece or in order.
    for (int a = 0; a < A; ++a) {
        volatile uint32_t* m = mbox_host(a);
        uint32_t sw3[3];
        memcpy(sw3, state + (size_t)a * 3, 12);
        const uint32_t tag = seq & 0xffffu;
        const uint16_t half[13] = {(uint16_t)step, (uint16_t)(step >> 16), (uint16_t)(add_noise != 0),
                                   (uint16_t)ip, (uint16_t)(ip >> 16), (uint16_t)(ip >> 32), (uint16_t)(ip >> 48),
                                   (uint16_t)sw3[0], (uint16_t)(sw3[0] >> 16), (uint16_t)sw3[1], (uint16_t)(sw3[1] >> 16),
                                   (uint16_t)sw3[2], (uint16_t)(sw3[2] >> 16)};
        for (int i = 0; i < 13; ++i) m[i] = ((uint32_t)half[i] << 16) | tag;
        m[15] = seq;
    }
    std::atomic_thread_fence(std::memory_order_release);
    // host work that hides under the kernel: the next chunk's noise, the previous call's collective
    if (pf_chunk[nb] != c + 1) {
        // the other buffer held chunk c-1: every control step that read it has handed its record to this thread already
        launch_noise_fill(c + 1, nb, pf_stream);
        HIP_CHECK(hipEventRecord(pf_done[nb], pf_stream));
        pf_chunk[nb] = c + 1; pf_waited[nb] = false; pf_inflight[nb] = true;
    }
    note_in_flight();
    const auto t0 = std::chrono::steady_clock::now();
    bool all = true;
    for (int a = 0; a < A; ++a) {
        volatile const uint32_t* ack = ack_host(a);              // the agent's completion line (completion_line.hpp)
        volatile const uint32_t* gone = gone_host(a);
        bool served = false;
        // also over when the agent's workgroup left (before or after this request?); after 2 s nobody is asked again
        spin_until(t0, [&] { return (served = completion_line_decode(ack, seq, records + (size_t)a * kCompletionRecordFloats)) || *gone != 0u; },
                   [] { return false; });
        if (!served) all = false;
    }
    if (all) return true;
    // some workgroups have left: end the others too (they finish the step they are in), then see who is missing
    resident_stop();
    int missing = 0;
    int32_t* amap = amap_host();
    for (int a = 0; a < A; ++a)
        if (!completion_line_decode(ack_host(a), seq, records + (size_t)a * kCompletionRecordFloats)) amap[missing++] = a;
    if (missing == 0) return true;                                // everybody took the request on the way out
    --step_counter;                                               // the launch that follows does this step ...
    subset_n = missing < A ? missing : 0;                         // ... for the agents that were not served (all of them: an ordinary launch)
    return false;
}

static void resident_unpublish(Engine* e) {
    if (e->mbox_pub.load(std::memory_order_relaxed)) {
        e->mbox_pub.store(nullptr, std::memory_order_release);
        g_resident_handles.fetch_sub(1, std::memory_order_relaxed);
    }
}

void Engine::resident_stop() {
    if (!resident_alive) return;
    resident_unpublish(this);
    for (int a = 0; a < A; ++a) mbox_host(a)[15] = 0xffffffffu;   // the stop word (word 15 alone decides)
    std::atomic_thread_fence(std::memory_order_release);
    resident_alive = false;
    HIP_CHECK(hipStreamSynchronize(stream));
}

float* Engine::pinned(size_t count) {
    if (count > h_pin_n) {
        invalidate_step_graph();             // a captured control step reads and writes the old buffer through h_pin_dev
        if (h_pin) (void)hipHostFree(h_pin);
        h_pin = nullptr;
        h_pin_n = 0;
        HIP_CHECK(hipHostMalloc((void**)&h_pin, count * sizeof(float), hipHostMallocCoherent | hipHostMallocMapped));
        h_pin_n = count;
        HIP_CHECK(hipHostGetDevicePointer((void**)&h_pin_dev, h_pin, 0));
    }
    return h_pin;
}

OptArgs Engine::opt_args(uint32_t step, uint32_t iter) const {
    OptArgs o;
    o.N = N; o.A = A; o.H = H; o.U = U; o.HU = HU; o.Nst = Nst;
    o.agent_offset = cfg.agent_offset;
    o.lo = d_lo.p; o.hi = d_hi.p;
    o.key = key(step);
    o.iter = iter;
    o.pop_offset = cfg.population_offset;
    return o;
}

PsoState Engine::pso_state(int shard) {
    PsoState s;
    const size_t big = (size_t)A * HU * Nst * shard, small = (size_t)A * Nst * shard;
    s.pos = d_cand_a.p + big; s.vel = d_vel.p + big; s.pbest = d_pbest.p + big; s.pbest_r = d_pbest_r.p + small;
    s.gbest = d_gbest.p; s.gbest_r = d_gbest_r.p; s.cond = d_cond.p + small; s.gidx = d_gidx.p;
    return s;
}


void Engine::reset() {
    carry_stored = 0;                              // bbmpc_set_elite_carry: the stored elites go, the setting stays
    // CEM/PI2/SPSA reset(): previous solution <- bounds midpoint (cem.py:138-149, pi2.py:98-105)
    if (cfg.optimizer == BBMPC_OPT_NONE || cfg.optimizer == BBMPC_OPT_RANDOM_SEARCH) return;
    cem_sigma0_ready = false;                      // (prev_mean is rewritten below)
    if (cfg.optimizer == BBMPC_OPT_CMAES) {          // restores m and sigma only (cma_es.py:215-227)
        HIP_CHECK(hipStreamSynchronize(stream));
        cma_reset_mean_sigma();
        return;
    }
    if (cfg.optimizer == BBMPC_OPT_PSO) {
        // PSOOptimizer.reset(): uniform positions / velocities, pbest = pos, rewards -inf  (pso.py:143-160)
        OptArgs oa = opt_args(step_counter, 0xFFFFu);
        for (int r = 0; r < (ps_loopback > 1 ? ps_loopback : 1); ++r) {
            if (ps_loopback > 1) oa.pop_offset = r * N;
            hipLaunchKernelGGL(k_pso_seed, dim3((N + 255) / 256, HU, A), dim3(256), 0, stream, oa, pso_state(r), d_var0.p,
                               cfg.pso_v0_fraction, 1, injected(BBMPC_NOISE_PSO_RESET_POS), injected(BBMPC_NOISE_PSO_RESET_VEL));
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    std::vector<float> m((size_t)A * HU);
    for (int i = 0; i < A * HU; ++i) m[i] = (lo[i % U] + hi[i % U]) / 2.0f;
    HIP_CHECK(hipMemcpyAsync(d_prev_mean.p, m.data(), m.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// ------------------------------------------------------------------------------------------------
// layout helpers (host)
// ------------------------------------------------------------------------------------------------
void Engine::to_internal(const float* ref, int n_pop, float* out) const {
    // [n,A,H,U] -> [A][HU][Nst]
    for (int n = 0; n < n_pop; ++n)
        for (int a = 0; a < A; ++a)
            for (int j = 0; j < HU; ++j) out[((size_t)a * HU + j) * Nst + n] = ref[((size_t)n * A + a) * HU + j];
}
void Engine::from_internal(const float* in, int n_pop, float* ref) const {
    for (int n = 0; n < n_pop; ++n)
        for (int a = 0; a < A; ++a)
            for (int j = 0; j < HU; ++j) ref[((size_t)n * A + a) * HU + j] = in[((size_t)a * HU + j) * Nst + n];
}

// ------------------------------------------------------------------------------------------------
// side streams
// ------------------------------------------------------------------------------------------------
// HIP multiplexes streams onto a few hardware queues (GPU_MAX_HW_QUEUES, default 4) and a process that also runs
// PyTorch / c10d easily holds more streams than that.  If the communication stream lands on the launch stream's queue
// its cross-stream wait serialises the two (record all-gather, config 2: 53.7 -> 70 us per control step, depending only
// on how many streams the process happened to create before).  Queues are pooled per priority, so the communication
// stream is created with the highest priority -- a latency-critical, tiny collective: 56-57 us whatever else the process
// creates.  (Do not combine with GPU_MAX_HW_QUEUES=8: measured 112 us.)  Round 2: ALL of a handle's streams (launch,
// noise prefetch, communication) are in that pool, three streams for its four queues, so that the resident control-step
// kernel never holds back PyTorch's or the caller's normal-priority work; between handles see stop_foreign_residents.
hipStream_t create_comm_stream() {
    int least = 0, greatest = 0;
    HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    hipStream_t s = nullptr;
    HIP_CHECK(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest));
    return s;
}

// ------------------------------------------------------------------------------------------------
// profiling (HIP events on the launch stream around the dominant kernel)
// ------------------------------------------------------------------------------------------------
void Engine::prof_begin() {
    prof_this = profiling && (prof_seq++ % (uint64_t)prof_every) == 0;
    if (!prof_this) return;
    if (ev_used + 2 > ev_pool.size()) {
        for (int i = 0; i < 2; ++i) {
            hipEvent_t e;
            HIP_CHECK(hipEventCreate(&e));
            ev_pool.push_back(e);
        }
    }
    HIP_CHECK(hipEventRecord(ev_pool[ev_used], stream));
}
void Engine::prof_end() {
    if (!prof_this) return;
    HIP_CHECK(hipEventRecord(ev_pool[ev_used + 1], stream));
    ev_used += 2;
}
void Engine::get_profile(double* ms, int64_t* launches) {
    HIP_CHECK(hipStreamSynchronize(stream));
    double tot = 0.0;
    for (size_t i = 0; i + 1 < ev_used; i += 2) {
        float t = 0.f;
        HIP_CHECK(hipEventElapsedTime(&t, ev_pool[i], ev_pool[i + 1]));
        tot += t;
    }
    *ms = tot;
    *launches = (int64_t)(ev_used / 2);
    ev_used = 0;
}


// Candidates of this optimizer iteration into the sample buffer: the draws that the fused built-in kernels make on the
// fly, for the rollouts that cannot (the user-function paths of bbmpc_user.hip).  SRC_REF / SRC_BUF: nothing to draw.
void Engine::draw_candidates(int mode, RolloutArgs& ra) {
    if (mode != SRC_UNIFORM && mode != SRC_TRUNC) return;
    REQUIRE(ra.samples, BBMPC_E_STATE, "user-function rollout: no sample buffer");
    dim3 grid((ra.n_pop + 255) / 256, A), block(256);
    if (mode == SRC_UNIFORM) hipLaunchKernelGGL(k_gen_candidates<SRC_UNIFORM>, grid, block, 0, stream, ra);
    else hipLaunchKernelGGL(k_gen_candidates<SRC_TRUNC>, grid, block, (size_t)2 * ra.HU * sizeof(float), stream, ra);
    HIP_CHECK(hipGetLastError());
}

// bbmpc_set_sampling_correlation.  Everything that can be refused is refused before the handle
// changes; the copy runs on the handle's stream and is waited for.
void Engine::set_sampling_correlation(const float* mix, int64_t count) {
    if (!mix) {
        REQUIRE(count == 0, BBMPC_E_INVALID, "sampling correlation: a null matrix goes with count 0 (it removes the matrix)");
        if (corr_installed) invalidate_step_graph();
        corr_installed = false;
        return;
    }
    REQUIRE(cfg.optimizer == BBMPC_OPT_CEM || cfg.optimizer == BBMPC_OPT_PI2, BBMPC_E_UNSUPPORTED,
            "sampling correlation with an optimizer other than CEM or PI2: only their candidates are truncated-normal draws around a mean");
    REQUIRE(!pop_sharded() && cfg.population_global <= N && auto_split <= 1, BBMPC_E_UNSUPPORTED,
            "sampling correlation with a sharded population: the sharded control steps draw inside their rollout kernels");
    REQUIRE(HU <= CORR_MAX_HU, BBMPC_E_UNSUPPORTED,
            "sampling correlation: planning_horizon * dim_u = " + std::to_string(HU) + " exceeds " + std::to_string(CORR_MAX_HU) +
                ", the most one wave's draws take of a CU's LDS (k_gen_candidates_corr's tile is H*U x 64 floats)");
    REQUIRE(count == (int64_t)H * H, BBMPC_E_INVALID,
            "sampling correlation: the matrix must be [planning_horizon, planning_horizon] = " + std::to_string((int64_t)H * H) + " floats");
    for (int64_t i = 0; i < count; ++i) REQUIRE(std::isfinite(mix[i]), BBMPC_E_INVALID, "sampling correlation: the matrix has a non-finite element");
    std::vector<int> row_end((size_t)H, 1);
    for (int t = 0; t < H; ++t)
        for (int s = H - 1; s >= 1; --s)
            if (mix[(size_t)t * H + s] != 0.0f) { row_end[t] = s + 1; break; }
    invalidate_step_graph();
    if (!d_corr_mix.p) { d_corr_mix.alloc((size_t)H * H); d_corr_end.alloc((size_t)H); }
    corr_installed = false;                        // (a failed copy must not leave half a matrix in use)
    HIP_CHECK(hipMemcpyAsync(d_corr_mix.p, mix, (size_t)H * H * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(d_corr_end.p, row_end.data(), (size_t)H * 4, hipMemcpyHostToDevice, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    corr_installed = true;
}

// The mixed candidates of this CEM / PI2 iteration into the sample buffer (kernels_corr.hpp): clipped for CEM, as drawn for
// PI2, whose rollout clips and charges the penalty itself.
void Engine::draw_candidates_corr(RolloutArgs& ra) {
    REQUIRE(ra.samples, BBMPC_E_STATE, "sampling correlation: no sample buffer");
    REQUIRE(ra.H == H && ra.HU == HU, BBMPC_E_INVALID, "internal: correlated draw horizon");
    const size_t lds = (size_t)HU * CORR_LANES * sizeof(float);
    dim3 grid((ra.n_pop + CORR_LANES - 1) / CORR_LANES, A), block(CORR_LANES);
    if (cfg.optimizer == BBMPC_OPT_CEM) {
        want_lds((const void*)k_gen_candidates_corr<true>, lds);
        hipLaunchKernelGGL(k_gen_candidates_corr<true>, grid, block, lds, stream, ra, (const float*)d_corr_mix.p, (const int*)d_corr_end.p, ra.mean, ra.sigma,
                           ra.lo, ra.hi, ra.samples);
    } else {
        want_lds((const void*)k_gen_candidates_corr<false>, lds);
        hipLaunchKernelGGL(k_gen_candidates_corr<false>, grid, block, lds, stream, ra, (const float*)d_corr_mix.p, (const int*)d_corr_end.p, ra.mean, ra.sigma,
                           ra.lo, ra.hi, ra.samples);
    }
    HIP_CHECK(hipGetLastError());
}

// bbmpc_set_elite_carry.  Everything that can be refused is refused before the handle changes; an
// accepted call drops the stored elites, so the next control step injects nothing into its first iteration.
void Engine::set_elite_carry(int keep, int shift) {
    if (keep == 0 && shift == 0) {
        if (carry_on()) invalidate_step_graph();
        carry_keep = carry_shift = carry_stored = 0;
        return;
    }
    REQUIRE(cfg.optimizer == BBMPC_OPT_CEM, BBMPC_E_UNSUPPORTED,
            "elite carry with an optimizer other than CEM: only CEM selects elites that the next iteration could take up again");
    REQUIRE(!pop_sharded() && cfg.population_global <= N && auto_split <= 1, BBMPC_E_UNSUPPORTED,
            "elite carry with a sharded population: the sharded control steps draw inside their rollout kernels");
    REQUIRE(keep >= 0 && shift >= 0, BBMPC_E_INVALID, "elite carry: keep and shift must not be negative");
    REQUIRE(keep <= k && shift <= k, BBMPC_E_INVALID,
            "elite carry: keep and shift must not exceed num_elite = " + std::to_string(k));
    REQUIRE(keep < N && shift < N, BBMPC_E_INVALID,
            "elite carry: keep and shift must be below population_size = " + std::to_string(N));
    REQUIRE(!prior_on() || (long)prior_K + std::max(keep, shift) < (long)N, BBMPC_E_INVALID,
            "elite carry: policy prior count + max(keep, shift) = " + std::to_string((long)prior_K + std::max(keep, shift)) +
                " must be below population_size = " + std::to_string(N));
    invalidate_step_graph();
    const size_t need = (size_t)A * HU * std::max(keep, shift);
    if (d_carry.n != need) {
        HIP_CHECK(hipStreamSynchronize(stream));   // (nothing may still read the buffer that is replaced)
        carry_keep = carry_shift = carry_stored = 0;   // (a failed allocation must not leave a setting without its buffer)
        d_carry.alloc(need);
    }
    carry_keep = keep; carry_shift = shift; carry_stored = 0;
}

// The first `count` sorted elites of the refit that has just run, out of the sample buffer into the carry buffer
// (kernels_elite_carry.hpp); shift: moved one planning step forward, the last step repeated.
void Engine::save_elites(int count, bool shift) {
    if (count <= 0) return;
    dim3 grid((HU * count + CARRY_THREADS - 1) / CARRY_THREADS, A), block(CARRY_THREADS);
    if (shift)
        hipLaunchKernelGGL(k_elite_save<true>, grid, block, 0, stream, HU, U, Nst, N, k, carry_stride(), count, (const int*)d_elites.p,
                           (const float*)d_samples.p, d_carry.p);
    else
        hipLaunchKernelGGL(k_elite_save<false>, grid, block, 0, stream, HU, U, Nst, N, k, carry_stride(), count, (const int*)d_elites.p,
                           (const float*)d_samples.p, d_carry.p);
    HIP_CHECK(hipGetLastError());
}

// [batch, U] actions in a dense block: the caller's own when they are, else gathered from rows astride apart
const float* Engine::dense_actions(const float* d_actions, int astride, int batch) {
    if (astride == U) return d_actions;
    if (d_step_act.n < (size_t)batch * U) d_step_act.alloc((size_t)batch * U);
    HIP_CHECK(hipMemcpy2DAsync(d_step_act.p, (size_t)U * 4, d_actions, (size_t)astride * 4, (size_t)U * 4, batch, hipMemcpyDeviceToDevice, stream));
    return d_step_act.p;
}

void Engine::launch_rollout(int mode, bool pen, RolloutArgs& ra) {
    // bbmpc_set_elite_carry (CEM): the candidates go to the sample buffer, the stored elites over its last columns
    const bool carry = carry_on() && cfg.optimizer == BBMPC_OPT_CEM && mode == SRC_TRUNC;
    // bbmpc_set_policy_prior_mlp (CEM): the policy's rollouts over the columns in front of the carried ones
    const bool prior = prior_on() && cfg.optimizer == BBMPC_OPT_CEM && mode == SRC_TRUNC;
    // bbmpc_set_grad_refine (CEM): gradient steps on the last columns, after everything else has formed them
    const bool grad = grad_on() && cfg.optimizer == BBMPC_OPT_CEM && mode == SRC_TRUNC;
    if ((corr_on() || carry || prior || grad) && mode == SRC_TRUNC) {      // bbmpc_set_sampling_correlation: mixed draws, then the SRC_BUF form
        if (corr_on()) draw_candidates_corr(ra);
        else draw_candidates(SRC_TRUNC, ra);
        if (prior) {
            const int c_i = carry ? carry_inject : 0;
            REQUIRE(ra.n_pop == N && ra.HU == HU && ra.H == H && ra.Nst == Nst && N - c_i - prior_K >= 0, BBMPC_E_INVALID, "internal: policy prior shape");
            policy_prior_rollouts(ra.state, prior_sigma != 0.0f ? policy_noise(ra.key.step, ra.iter) : nullptr, ra.samples, Nst,
                                  N - c_i - prior_K, nullptr, nullptr);
        }
        if (carry && carry_inject > 0) {
            REQUIRE(ra.n_pop == N && ra.HU == HU && ra.Nst == Nst && carry_inject < N && d_carry.p, BBMPC_E_INVALID, "internal: elite carry shape");
            hipLaunchKernelGGL(k_elite_inject, dim3((HU * carry_inject + CARRY_THREADS - 1) / CARRY_THREADS, A), dim3(CARRY_THREADS), 0, stream, HU, Nst,
                               N, carry_stride(), carry_inject, (const float*)d_carry.p, ra.samples);
            HIP_CHECK(hipGetLastError());
        }
        if (grad) grad_refine_candidates(ra);
        mode = SRC_BUF;
        ra.cand = ra.samples;
    }
    if (particles_on()) {                                 // bbmpc_set_particles: noisy rollouts + aggregate (bbmpc_particles.hip)
        rollout_particles(mode, pen, ra, nullptr, 0);
        return;
    }
    if (shaping_on()) {                                   // bbmpc_set_return_shaping: recording on, every sequence ends in k_shaped_return
        dominant_kernel = "k_rollout_mlp";
        rollout_shaped(mode, pen, ra);
        return;
    }
    if (value_on()) {                                     // a learned terminal value: today's rollout with recording on + one launch
        dominant_kernel = "k_rollout_mlp";
        rollout_terminal_value(mode, pen, ra);
        return;
    }
    if (cfg.reward == BBMPC_REW_MLP) {                    // a learned reward: MFMA rollout + MFMA scorer, whatever BBMPC_USER_STEPWISE says
        dominant_kernel = "k_rollout_mlp";
        rollout_mlp_reward_mlp(mode, pen, ra);
        return;
    }
    if (user_path()) {
        if (user_callbacks()) {                           // a host callback per planning step: step-wise only
            dominant_kernel = "stepwise(user callback)";
            rollout_stepwise(mode, pen, ra);
        } else if (cfg.dynamics != BBMPC_DYN_MLP && !user_stepwise_only) {
            dominant_kernel = "bbmpc_user_rollout(hiprtc)";
            rollout_user_fused(mode, pen, ra);
        } else if (cfg.dynamics == BBMPC_DYN_MLP && !user_stepwise_only && has_xform()) {
            dominant_kernel = "bbmpc_mlp_xform_rollout(hiprtc)";
            rollout_mlp_xform(mode, pen, ra);
        } else if (cfg.dynamics == BBMPC_DYN_MLP && !user_stepwise_only) {
            dominant_kernel = "k_rollout_mlp";
            rollout_mlp_user_reward(mode, pen, ra);
        } else {
            dominant_kernel = "stepwise(user device function)";
            rollout_stepwise(mode, pen, ra);
        }
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_MLP) {
        dominant_kernel = "k_rollout_mlp";
        launch_rollout_mlp(mode, pen, ra, false, nullptr, nullptr);
        return;
    }
    // few trajectories -> one wave per workgroup so every wave gets its own SIMD (latency);
    // many -> 256-thread workgroups.
    const int bs = ((long)ra.n_pop * A <= 16384) ? 64 : 256;
    dim3 grid((ra.n_pop + bs - 1) / bs, A), block(bs);
    prof_begin();
    const bool fm = !fix(BBMPC_STRICT_MATH);
    const size_t lds_ms = (size_t)2 * HU * sizeof(float);
#define LAUNCH_ROLL(M, P, L)                                                                               \
    do {                                                                                                   \
        if (fm) hipLaunchKernelGGL((k_rollout_pendulum<M, P, true>), grid, block, (L), stream, ra);       \
        else hipLaunchKernelGGL((k_rollout_pendulum<M, P, false>), grid, block, (L), stream, ra);         \
    } while (0)
    if (mode == SRC_REF) LAUNCH_ROLL(SRC_REF, false, (size_t)bs * 33 * sizeof(float));
    else if (mode == SRC_UNIFORM) LAUNCH_ROLL(SRC_UNIFORM, false, 0);
    else if (mode == SRC_TRUNC && !pen) LAUNCH_ROLL(SRC_TRUNC, false, lds_ms);
    else if (mode == SRC_TRUNC && pen) LAUNCH_ROLL(SRC_TRUNC, true, lds_ms);
    else if (mode == SRC_BUF) LAUNCH_ROLL(SRC_BUF, true, 0);
    else throw HipError(BBMPC_E_INVALID, "bad rollout mode");
#undef LAUNCH_ROLL
    HIP_CHECK(hipGetLastError());
    prof_end();
}

void Engine::ensure_trace() {
    const size_t nr = (size_t)A * Nst, nm = (size_t)A * HU, ns = (size_t)A * HU * Nst, ne = (size_t)A * std::max(k, 1);
    const int nit = std::max(iters, 1);
    if (!t_rewards.p) {
        t_rewards.alloc(nr * nit);
        t_mean.alloc(nm * nit);
        t_var.alloc(nm * nit);
        t_samples.alloc(ns * nit);
        t_elites.alloc(ne * nit);
        t_passes.alloc((size_t)A * nit);
        HIP_CHECK(hipMemsetAsync(t_passes.p, 0, (size_t)A * nit * 4, stream));
    }
}

void Engine::capture_trace(int it) {
    if (!trace_on) return;
    const size_t nr = (size_t)A * Nst, nm = (size_t)A * HU, ns = (size_t)A * HU * Nst, ne = (size_t)A * std::max(k, 1);
    ensure_trace();
    HIP_CHECK(hipMemcpyAsync(t_rewards.p + nr * it, d_rewards.p, nr * 4, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(t_mean.p + nm * it, d_mean.p, nm * 4, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(t_var.p + nm * it, d_var.p, nm * 4, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(t_samples.p + ns * it, d_samples.p, ns * 4, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpyAsync(t_elites.p + ne * it, d_elites.p, ne * 4, hipMemcpyDeviceToDevice, stream));
}


void Engine::finalize(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out, uint32_t step) {
    FinalArgs fa;
    fa.A = A; fa.U = U; fa.S = S;
    fa.agent_offset = cfg.agent_offset;
    fa.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    fa.fix_q7 = fix(BBMPC_FIX_Q7_EXPL_NOISE_ZERO_MEAN);
    fa.add_noise = add_noise;
    fa.state = d_state_in;
    fa.action = d_action.p;
    fa.lo = d_lo.p; fa.hi = d_hi.p;
    fa.inj = injected(BBMPC_NOISE_EXPLORATION);
    fa.record = d_record_out;
    fa.next_state = d_next_out;
    fa.key = key(step);
    fa.key.q_per_agent = (uint32_t)((U + 3) / 4);
    if (pending_cma_update.set) {                     // (analytic pendulum, CMA-ES at n <= 32: bbmpc_cma.hip)
        launch_pending_cma_update(fa);
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_PENDULUM && !user_path()) {
        const TailHandoff::Words w = tail.publish_words();   // the record is complete when this kernel ends: it publishes the sequence number
        hipLaunchKernelGGL(k_finalize_pendulum, dim3((A + 63) / 64), dim3(64), 0, stream, fa, w.flag, w.count, w.value);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (user_path()) {
        // a user device function is involved: exploration noise, one batched model step + reward on the [A] rows, pack
        if (add_noise) {
            hipLaunchKernelGGL(k_explore, dim3((A * U + 63) / 64), dim3(64), 0, stream, fa, d_action.p);
            HIP_CHECK(hipGetLastError());
        }
        if (!d_fin_next.p) {
            d_fin_next.alloc((size_t)A * S);
            d_fin_rew.alloc((size_t)((A + 63) / 64) * 64);
        }
        step_dev(d_state_in, d_action.p, U, A, d_fin_next.p, d_fin_rew.p);
        hipLaunchKernelGGL(k_pack_record, dim3((A * rec + 63) / 64), dim3(64), 0, stream, A, U, S, d_action.p, d_fin_next.p,
                           d_fin_rew.p, d_record_out, d_next_out);
        HIP_CHECK(hipGetLastError());
        if (pending_warm == 1) hipLaunchKernelGGL(k_shift_left, dim3((A * HU + 255) / 256), dim3(256), 0, stream, A, H, U, d_mean.p, d_prev_mean.p);
        else if (pending_warm == 2) HIP_CHECK(hipMemcpyAsync(d_prev_mean.p, d_mean.p, (size_t)A * HU * 4, hipMemcpyDeviceToDevice, stream));
        HIP_CHECK(hipGetLastError());
        pending_warm = 0;
        return;
    }
    // learned dynamics: exploration noise, one model step on the [A] rows, reward, packed record and the warm start of
    // the next control step in ONE launch (kernels_tail.hpp; was k_explore + k_step_mlp + k_pack_record + k_shift_left)
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    TailArgs ta;
    memset(&ta, 0, sizeof(ta));
    ta.f = fa;
    ta.net = row_mlp();
    ta.reward_kind = builtin_reward_kind();
    ta.warm_mode = pending_warm;
    ta.H = H; ta.HU = HU;
    ta.mean = d_mean.p;
    ta.prev_mean = d_prev_mean.p;
    pending_warm = 0;
    tail.publish_into(ta);       // the record is complete when this kernel ends: it publishes the sequence number itself
    if (tail.flag) ta.step_words = step_capturing ? step_words_dev : nullptr;
    launch_with_tail(*this, k_tail_mlp, dim3(A), dim3(TAIL_THREADS), 0, ta);
    HIP_CHECK(hipGetLastError());
}

RowMlp Engine::row_mlp() const {
    RowMlp r;
    memset(&r, 0, sizeof(r));
    r.m = mlp;
    for (int l = 0; l < mlp.n_layers; ++l) { r.wraw[l] = d_wraw[l].p; r.braw[l] = d_braw[l].p; }
    return r;
}


void Engine::optimize_dev(const float* d_state_in, int add_noise, float* d_record_out, float* d_next_out) {
    REQUIRE(cfg.optimizer != BBMPC_OPT_NONE, BBMPC_E_STATE, "handle was created without an optimizer");
    const uint32_t step = step_counter++;
    if (keep_plan) plan_ready = true;
    pending_cma_update.set = false;
    if (use_fused()) {
        dominant_kernel = "k_fused_pendulum";
        optimize_fused(d_state_in, add_noise, d_record_out, d_next_out, step);
        return;
    }
    if (use_fused_pso()) {
        dominant_kernel = "k_fused_pso_pendulum";
        optimize_fused_pso(d_state_in, add_noise, d_record_out, d_next_out, step);
        return;
    }
    if (use_fused_cma()) {
        dominant_kernel = "k_fused_cma_pendulum";
        optimize_fused_cma(d_state_in, add_noise, d_record_out, d_next_out, step);
        return;
    }
    dominant_kernel = "k_rollout_pendulum";
    RolloutArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.n_pop = N; ra.A = A; ra.H = H; ra.U = U; ra.S = S; ra.HU = HU; ra.Nst = Nst;
    ra.agent_offset = cfg.agent_offset;
    ra.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    ra.reward_kind = builtin_reward_kind();
    ra.state = d_state_in;
    ra.mean = d_mean.p; ra.sigma = d_sigma.p;
    ra.lo = d_lo.p; ra.hi = d_hi.p;
    ra.samples = d_samples.p;
    ra.rewards = d_rewards.p;
    ra.penalty_out = d_penalty.p;
    ra.key = key(step);
    ra.pop_offset = cfg.population_offset;
    switch (cfg.optimizer) {
        case BBMPC_OPT_RANDOM_SEARCH: optimize_random_search(ra); break;
        case BBMPC_OPT_CEM: optimize_cem(ra); break;
        case BBMPC_OPT_PI2: optimize_pi2(ra); break;
        case BBMPC_OPT_SPSA: optimize_spsa(ra, step); break;
        case BBMPC_OPT_PSO: optimize_pso(ra, step); break;
        case BBMPC_OPT_CMAES: optimize_cma(ra, step); break;
        default: throw HipError(BBMPC_E_UNSUPPORTED, "optimizer not built yet");
    }
    finalize(d_state_in, add_noise, d_record_out, d_next_out, step);
}

// ps_part of every rank -> ps_all.  The exchange sits ON the launch stream: the merge needs it, nothing can overlap it.
// A sharded code path without a communicator (BBMPC_POPSHARD_FORCE on one handle) has only its own payload to hand over.
void Engine::gather_shards(size_t pw, const char* what) {
    if (ps_loopback > 1) return;                   // play_shards wrote every shard's slot itself
    if (rc.comm) {
        const Rccl& r = *rc.api;
        r.check(r.AllGather(ps_part.p, ps_all.p, pw, Rccl::kFloat32, rc.comm, stream), what);
    } else {
        REQUIRE(cfg.population_global <= N, BBMPC_E_STATE, "population sharding needs a communicator: call bbmpc_comm_init first");
        HIP_CHECK(hipMemcpyAsync(ps_all.p, ps_part.p, pw * 4, hipMemcpyDeviceToDevice, stream));
    }
}

RefitArgs Engine::refit_args() const {
    RefitArgs rf;
    memset(&rf, 0, sizeof(rf));
    rf.N = N; rf.A = A; rf.H = H; rf.U = U; rf.HU = HU; rf.Nst = Nst; rf.k = k;
    rf.alpha = cfg.alpha;
    rf.inv_lamda = 1.0f / cfg.lamda;
    rf.rewards = d_rewards.p; rf.samples = d_samples.p;
    rf.lo = d_lo.p; rf.hi = d_hi.p;
    rf.mean = d_mean.p; rf.var = d_var.p; rf.sigma = d_sigma.p;
    rf.elites = d_elites.p; rf.action = d_action.p;
    return rf;
}

// Learned model on the quad kernel (k_rollout_mlp_q4s), CEM and PI2: from the second control step on k_dist_init (4.3 us, a
// launch of its own in front of a 360 us control step) has nothing left to do when the distribution the first rollout
// samples from is a constant of the handle -- the rollout samples from the constants directly and reads the state from the
// pinned buffer itself (its workgroup 0 stores it for the later launches).  What else must hold is the optimizer's own.
bool Engine::dist_init_skippable() const {
    return sw.pi2_skip_init && cfg.dynamics == BBMPC_DYN_MLP && !user_path() && !value_on() && !shaping_on() && !pop_sharded() && !trace_on && !particles_on() && !corr_on() && !carry_on() && !prior_on() && !grad_on() &&
           iters >= 1 && pi2_copy_seen && stage_state_src != nullptr;
}

// The first rollout of a learned-model CEM / PI2 control step; returns whether the kernel took the request to store the
// state.  pinned_state != null: k_dist_init was skipped, so this one launch samples from (mean, sigma; sigma == null: the
// handle's) and reads the state from the pinned buffer.  Otherwise the request only asks whether the kernel would take it.
bool Engine::first_rollout_mlp(bool pen, RolloutArgs& ra, const float* mean, const float* sigma, const float* pinned_state) {
    const float *mean_it = ra.mean, *sigma_it = ra.sigma, *state_it = ra.state;
    if (pinned_state) {
        ra.mean = mean; ra.state = pinned_state;
        if (sigma) ra.sigma = sigma;
    }
    mlp_state_copy = d_state.p;
    launch_rollout(SRC_TRUNC, pen, ra);
    const bool took = mlp_state_copy == nullptr;
    mlp_state_copy = nullptr;
    pi2_copy_seen = took;
    if (pinned_state) {
        if (!took)                                       // a shape the quad kernel refused after all: nobody stored the state
            HIP_CHECK(hipMemcpyAsync(d_state.p, pinned_state, (size_t)A * S * 4, hipMemcpyDefault, stream));
        ra.mean = mean_it; ra.sigma = sigma_it; ra.state = state_it;
    }
    return took;
}

// RandomSearchOptimizer._optimize  random_search.py:38-48
void Engine::optimize_random_search(RolloutArgs& ra) {
    const RefitArgs rf = refit_args();
    ra.stream = BBMPC_NOISE_UNIFORM; ra.iter = 0;
    ra.inj = injected(BBMPC_NOISE_UNIFORM);
    if (pop_sharded()) {
        // population sharded over ranks: local first maximum, one exchange, first maximum by global index
        const size_t pw = (size_t)A * (U + 2);
        shard_buffers(pw);
        play_shards(pw, ra.pop_offset, [&](int pop_offset, float* part) {
            launch_rollout(SRC_UNIFORM, false, ra);
            hipLaunchKernelGGL(k_refit_argmax, dim3(A), dim3(REFIT_THREADS), 0, stream, rf, part, pop_offset);
        });
        gather_shards(pw, "ncclAllGather (RandomSearch local bests)");
        HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(k_argmax_merge, dim3(A), dim3(64), 0, stream, rf, ps_all.p, shard_count());
        HIP_CHECK(hipGetLastError());
        capture_trace(0);
        return;
    }
    launch_rollout(SRC_UNIFORM, false, ra);
    hipLaunchKernelGGL(k_refit_argmax, dim3(A), dim3(REFIT_THREADS), 0, stream, rf, (float*)nullptr, 0);
    HIP_CHECK(hipGetLastError());
    capture_trace(0);
}

// CEMOptimizer._optimize  cem.py:74-136
void Engine::optimize_cem(RolloutArgs& ra) {
    const RefitArgs rf = refit_args();
    const int nelem = A * HU;
    // The reference's restart from the constructor distribution every control step (no BBMPC_FIX_Q2_CEM_WARM_START):
    // prev_mean, var0 and the sigma they give are constants, so k_dist_init can be skipped (dist_init_skippable) -- the
    // first rollout samples from (prev_mean, sigma0), the first refit smooths against (prev_mean, var0)
    const bool cem_skip = dist_init_skippable() && k <= 64 && !sw.refit_v1 && !fix(BBMPC_FIX_Q2_CEM_WARM_START) && cem_sigma0_ready;
    const float* cem_pinned = nullptr;
    last_step_steady = cem_skip;
    if (cem_skip) {
        cem_pinned = stage_state_src;
    } else {
        hipLaunchKernelGGL(k_dist_init, dim3((nelem + 255) / 256), dim3(256), 0, stream, A, HU, U, d_lo.p, d_hi.p,
                           d_prev_mean.p, d_var0.p, d_mean.p, d_var.p, d_sigma.p, 1, stage_state_src, d_state.p, A * S);
        if (!cem_sigma0_ready && !fix(BBMPC_FIX_Q2_CEM_WARM_START)) {
            if (!step_capturing) invalidate_step_graph();   // (a replayed control step samples from d_sigma0: never capture across its allocation)
            d_sigma0.alloc(nelem);
            HIP_CHECK(hipMemcpyAsync(d_sigma0.p, d_sigma.p, (size_t)nelem * 4, hipMemcpyDeviceToDevice, stream));
            cem_sigma0_ready = true;
        }
    }
    stage_state_src = nullptr;
    // iters == 0: action = mean[:,0] of the untouched distribution (otherwise the last refit writes it)
    if (iters == 0)
        HIP_CHECK(hipMemcpy2DAsync(d_action.p, U * 4, d_prev_mean.p, HU * 4, U * 4, A, hipMemcpyDeviceToDevice, stream));
    const float* inj_t = injected(BBMPC_NOISE_TRUNC_NORMAL);
    const size_t inj_stride = (size_t)A * HU * Nst;
    if (trace_on) ensure_trace();                         // (the refit kernels store their pass counts into the trace itself)
    // LDS budget for the refit: rewards + elite idx + elite tile
    const int kpad = (k + 3) & ~3;
    const int fixed = Nst + kpad + TOPK_HIST_WORDS + 2 * kpad;
    const int budget = fixed * 4 > 48 * 1024 ? 158 * 1024 / 4 : 62 * 1024 / 4;     // floats; big populations take the whole LDS
    int JC = (int)((size_t)std::max(budget - fixed, k) / (size_t)k);
    JC = std::max(1, std::min(JC, HU));
    const size_t lds = (size_t)(fixed + (size_t)k * JC) * 4;
    want_lds((const void*)k_refit_cem_v2, (size_t)fixed * 4);
    want_lds((const void*)k_refit_cem, lds);
    // bbmpc_set_elite_carry: what the previous control step left goes into iteration 0 and is then used up
    const bool carry = carry_on() && !pop_sharded();
    const int carry_first = carry ? carry_stored : 0;
    if (carry) carry_stored = 0;
    for (int it = 0; it < iters; ++it) {
        ra.stream = BBMPC_NOISE_TRUNC_NORMAL; ra.iter = (uint32_t)it;
        carry_inject = !carry ? 0 : (it == 0 ? carry_first : carry_keep);
        ra.inj = inj_t ? inj_t + inj_stride * it : nullptr;
        if (pop_sharded()) {
            // population sharded over ranks: local top-k + rows, one exchange, global top-k + refit
            const int G = shard_count();
            const size_t pw = (size_t)A * k * (HU + 2);
            shard_buffers(pw);
            const size_t tl = (size_t)fixed * 4;
            want_lds((const void*)k_cem_local_topk, tl);
            const int psg = sw.refit_wgs > 0 ? sw.refit_wgs : std::max(1, std::min(8, HU / 16));   // workgroups per agent (kernels_tail.hpp)
            RefitArgs rfs = rf;
            if (!trace_on) rfs.elites = nullptr;
            play_shards(pw, ra.pop_offset, [&](int pop_offset, float* part) {
                launch_rollout(SRC_TRUNC, false, ra);
                hipLaunchKernelGGL(k_cem_local_topk, dim3(psg, A), dim3(1024), tl, stream, rf, pop_offset, part);
            });
            gather_shards(pw, "ncclAllGather (CEM local elites)");
            HIP_CHECK(hipGetLastError());
            const size_t ml = ((size_t)2 * G * k + k) * 4;
            want_lds((const void*)k_cem_merge, ml);
            hipLaunchKernelGGL(k_cem_merge, dim3(psg, A), dim3(256), ml, stream, rfs, ps_all.p, G);
            HIP_CHECK(hipGetLastError());
            capture_trace(it);
            continue;
        }
        bool first_from_constants = false;
        if (it == 0 && cfg.dynamics == BBMPC_DYN_MLP && !user_path() && !value_on() && !shaping_on() && !grad_on()) {
            first_rollout_mlp(false, ra, d_prev_mean.p, d_sigma0.p, cem_pinned);
            first_from_constants = cem_skip;
        } else {
            launch_rollout(SRC_TRUNC, false, ra);
        }
        if (k <= 64 && !sw.refit_v1) {
            const int rthreads = N > 512 ? 1024 : (N > 256 ? 512 : 256);
            RefitArgs rf2 = rf;
            rf2.passes = trace_on ? t_passes.p + (size_t)A * it : nullptr;
            if (!trace_on && !carry) rf2.elites = nullptr;   // the sorted elite list is only needed by the parity trace and the elite carry
            if (first_from_constants) { rf2.mean_in = d_prev_mean.p; rf2.var_in = d_var0.p; }
            // G workgroups per agent share the elite gather (kernels_refit.hpp); at least 16 rows each
            const int rg = sw.refit_wgs > 0 ? sw.refit_wgs : std::max(1, std::min(8, HU / 16));
            hipLaunchKernelGGL(k_refit_cem_v2, dim3(rg, A), dim3(rthreads), (size_t)fixed * 4, stream, rf2);
        } else {
            RefitArgs rf1 = rf;
            rf1.passes = trace_on ? t_passes.p + (size_t)A * it : nullptr;
            hipLaunchKernelGGL(k_refit_cem, dim3(A), dim3(REFIT_THREADS), lds, stream, rf1, JC);
        }
        HIP_CHECK(hipGetLastError());
        if (carry) {                                      // the elite rows leave the sample buffer before the next draw rewrites it
            if (it + 1 < iters) save_elites(carry_keep, false);
            else { save_elites(carry_shift, true); carry_stored = carry_shift; }
        }
        capture_trace(it);
    }
    carry_inject = 0;
    if (fix(BBMPC_FIX_Q2_CEM_WARM_START)) {
        if (cfg.dynamics == BBMPC_DYN_MLP || user_path()) pending_warm = 2;      // prev = mean, in k_tail_mlp
        else HIP_CHECK(hipMemcpyAsync(d_prev_mean.p, d_mean.p, (size_t)nelem * 4, hipMemcpyDeviceToDevice, stream));
    }
}

// PI2Optimizer._optimize  pi2.py:58-96
void Engine::optimize_pi2(RolloutArgs& ra) {
    const RefitArgs rf = refit_args();
    const int nelem = A * HU;
    // PI2 never changes sigma, the first rollout samples around prev_mean directly and the refit writes every element of
    // the mean: k_dist_init can be skipped (dist_init_skippable) once it has run
    const bool skip_init = dist_init_skippable() && pi2_dist_ready;
    const float* pinned_state = nullptr;
    last_step_steady = skip_init;
    if (skip_init) {
        pinned_state = stage_state_src;
    } else {
        hipLaunchKernelGGL(k_dist_init, dim3((nelem + 255) / 256), dim3(256), 0, stream, A, HU, U, d_lo.p, d_hi.p,
                           d_prev_mean.p, d_var0.p, d_mean.p, d_var.p, d_sigma.p, 0, stage_state_src, d_state.p, A * S);
        pi2_dist_ready = true;
    }
    stage_state_src = nullptr;
    if (iters == 0)              // otherwise the last refit writes the action
        HIP_CHECK(hipMemcpy2DAsync(d_action.p, U * 4, d_prev_mean.p, HU * 4, U * 4, A, hipMemcpyDeviceToDevice, stream));
    const float* inj_t = injected(BBMPC_NOISE_TRUNC_NORMAL);
    const size_t inj_stride = (size_t)A * HU * Nst;
    const size_t lds = (size_t)(Nst + 64) * 4;
    want_lds((const void*)k_refit_pi2_mw, lds);
    want_lds((const void*)k_refit_pi2, lds);
    want_lds((const void*)k_refit_pi2_partial, lds);
    for (int it = 0; it < iters; ++it) {
        ra.stream = BBMPC_NOISE_TRUNC_NORMAL; ra.iter = (uint32_t)it;
        ra.inj = inj_t ? inj_t + inj_stride * it : nullptr;
        if (pop_sharded()) {
            // population sharded over ranks: partial sums here, one exchange, merge in rank order
            const size_t pw = (size_t)A * (HU + 2);
            shard_buffers(pw);
            dim3 pgrid((HU + PI2_ROWS - 1) / PI2_ROWS, A), pblock(64 * PI2_ROWS);
            play_shards(pw, ra.pop_offset, [&](int, float* part) {
                launch_rollout(SRC_TRUNC, true, ra);
                hipLaunchKernelGGL(k_refit_pi2_partial, pgrid, pblock, lds, stream, rf, part);
            });
            gather_shards(pw, "ncclAllGather (PI2 partials)");
            HIP_CHECK(hipGetLastError());
            hipLaunchKernelGGL(k_refit_pi2_merge, dim3((HU + 255) / 256, A), dim3(256), 0, stream, rf, ps_all.p, shard_count());
            HIP_CHECK(hipGetLastError());
            capture_trace(it);
            continue;
        }
        if (it == 0 && cfg.dynamics == BBMPC_DYN_MLP && !user_path() && !value_on() && !shaping_on()) first_rollout_mlp(true, ra, d_prev_mean.p, nullptr, pinned_state);
        else launch_rollout(SRC_TRUNC, true, ra);
        if (sw.refit_v1) hipLaunchKernelGGL(k_refit_pi2, dim3(A), dim3(REFIT_THREADS), lds, stream, rf);
        else hipLaunchKernelGGL(k_refit_pi2_mw, dim3((HU + PI2_ROWS - 1) / PI2_ROWS, A), dim3(64 * PI2_ROWS), lds, stream, rf);
        HIP_CHECK(hipGetLastError());
        capture_trace(it);
    }
    if (cfg.dynamics == BBMPC_DYN_MLP || user_path()) {
        pending_warm = 1;                      // prev = shift_left(mean) (pi2.py:92-93) happens in k_tail_mlp
    } else {
        hipLaunchKernelGGL(k_shift_left, dim3((nelem + 255) / 256), dim3(256), 0, stream, A, H, U, d_mean.p, d_prev_mean.p);
        HIP_CHECK(hipGetLastError());
    }
}


// SPSAOptimizer._optimize  spsa.py:61-117
void Engine::optimize_spsa(RolloutArgs& ra, uint32_t step) {
    const int nelem = A * HU;
    // solution starts from _current_parameters (d_prev_mean); keep it in d_mean while iterating
    HIP_CHECK(hipMemcpyAsync(d_mean.p, d_prev_mean.p, (size_t)nelem * 4, hipMemcpyDeviceToDevice, stream));
    HIP_CHECK(hipMemcpy2DAsync(d_action.p, U * 4, d_prev_mean.p, HU * 4, U * 4, A, hipMemcpyDeviceToDevice, stream));
    const float* inj_r = injected(BBMPC_NOISE_RADEMACHER);
    const size_t inj_stride = (size_t)A * HU * Nst;
    const float big_a = (float)iters / 10.0f;                                   // spsa.py:56
    for (int it = 0; it < iters; ++it) {
        const float tf = (float)it;
        const float ak = cfg.spsa_a / (float)pow((double)((tf + 1.0f) + big_a), (double)cfg.spsa_alpha);   // :69
        const float ck = cfg.spsa_c / (float)pow((double)(tf + 1.0f), (double)cfg.spsa_gamma);             // :70
        OptArgs oa = opt_args(step, (uint32_t)it);
        if (particles_on()) ra.iter = (uint32_t)it;       // the process noise is drawn per iteration
        want_lds((const void*)k_refit_spsa, (size_t)Nst * 4);
        // candidates -> the two rollouts -> row sums of this handle's perturbation pairs (part != null: sharded population;
        // the population offset is oa's)
        auto shard_pass = [&](int, float* part) {
            hipLaunchKernelGGL(k_spsa_candidates, dim3((N + 255) / 256, HU, A), dim3(256), 0, stream, oa, d_mean.p, ck,
                               inj_r ? inj_r + inj_stride * it : nullptr, d_samples.p, d_cand_a.p, d_cand_b.p);
            HIP_CHECK(hipGetLastError());
            ra.samples = nullptr;              // candidates are clipped in place; delta lives in d_samples
            ra.penalty_out = nullptr;
            ra.cand = d_cand_a.p; ra.samples = d_cand_a.p; ra.rewards = d_rewards.p;
            launch_rollout(SRC_BUF, true, ra);
            ra.cand = d_cand_b.p; ra.samples = d_cand_b.p; ra.rewards = d_rewards2.p;
            launch_rollout(SRC_BUF, true, ra);
            const int rgr = std::max(1, std::min(16, HU / (REFIT_THREADS / 64)));        // workgroups per agent: >= one row per wave
            hipLaunchKernelGGL(k_refit_spsa, dim3(rgr, A), dim3(REFIT_THREADS), (size_t)Nst * 4, stream, oa, d_rewards.p, d_rewards2.p,
                               d_samples.p, ak, ck, d_mean.p, d_action.p, part);
            HIP_CHECK(hipGetLastError());
        };
        if (pop_sharded()) {
            // population sharded over ranks: row sums here, one exchange, the step in rank order (kernels_opt.hpp)
            const int G = shard_count();
            const size_t pw = (size_t)A * HU;
            shard_buffers(pw);
            play_shards(pw, oa.pop_offset, shard_pass);
            gather_shards(pw, "ncclAllGather (SPSA row sums)");
            const int n_global = ps_loopback > 1 ? G * N : std::max(N, (int)cfg.population_global);
            hipLaunchKernelGGL(k_spsa_merge, dim3((HU + 255) / 256, A), dim3(256), 0, stream, oa, ps_all.p, G, n_global, ak, d_mean.p, d_action.p);
            HIP_CHECK(hipGetLastError());
        } else {
            shard_pass(oa.pop_offset, nullptr);
        }
        if (trace_on) {
            capture_trace(it);
            if (!t_rewards2.p) t_rewards2.alloc((size_t)A * Nst * std::max(iters, 1));
            HIP_CHECK(hipMemcpyAsync(t_rewards2.p + (size_t)A * Nst * it, d_rewards2.p, (size_t)A * Nst * 4,
                                     hipMemcpyDeviceToDevice, stream));
        }
    }
    if (cfg.dynamics == BBMPC_DYN_MLP || user_path()) {
        pending_warm = 1;                              // :114-115, in k_tail_mlp
    } else {
        hipLaunchKernelGGL(k_shift_left, dim3((nelem + 255) / 256), dim3(256), 0, stream, A, H, U, d_mean.p, d_prev_mean.p);  // :114-115
        HIP_CHECK(hipGetLastError());
    }
}


// PSOOptimizer._optimize  pso.py:70-141
void Engine::optimize_pso(RolloutArgs& ra, uint32_t step) {
    PsoState ps = pso_state();
    const float* inj_s = injected(BBMPC_NOISE_PSO_SCALARS);
    // population sharded over ranks: every rank moves ITS particles; the one cross-particle operation, the
    // argmax of the personal bests (pso.py:94), becomes local best -> all-gather -> first maximum by global index
    const bool sharded = pop_sharded();
    const int G = sharded ? shard_count() : 1;
    const int shards_here = ps_loopback > 1 ? ps_loopback : 1;         // the loopback hook plays every shard in turn
    const size_t pw = (size_t)A * (HU + 2);
    if (sharded) shard_buffers(pw);
    for (int it = 0; it < iters; ++it) {
        OptArgs oa = opt_args(step, (uint32_t)it);
        if (particles_on()) ra.iter = (uint32_t)it;       // the process noise is drawn per iteration
        for (int r = 0; r < shards_here; ++r) {
            const PsoState pr = pso_state(r);
            if (ps_loopback > 1) oa.pop_offset = r * N;
            ra.cand = pr.pos; ra.samples = pr.pos; ra.rewards = d_rewards.p; ra.penalty_out = nullptr;
            launch_rollout(SRC_BUF, true, ra);                 // clip + penalty + write the feasible positions back
            hipLaunchKernelGGL(k_pso_best, dim3(A), dim3(REFIT_THREADS), 0, stream, oa, pr, d_rewards.p,
                               !sharded ? nullptr : (ps_loopback > 1 ? ps_all.p + pw * r : ps_part.p));
            HIP_CHECK(hipGetLastError());
        }
        if (sharded) {
            gather_shards(pw, "ncclAllGather (PSO local bests)");
            hipLaunchKernelGGL(k_pso_merge, dim3(A), dim3(256), 0, stream, oa, ps, ps_all.p, G);
            HIP_CHECK(hipGetLastError());
        }
        for (int r = 0; r < shards_here; ++r) {
            hipLaunchKernelGGL(k_pso_move, dim3((N + 255) / 256, HU, A), dim3(256), 0, stream, oa, pso_state(r), cfg.pso_w, cfg.pso_c1,
                               cfg.pso_c2, inj_s ? inj_s + 2 * it : nullptr);
            HIP_CHECK(hipGetLastError());
        }
        if (trace_on) {
            ensure_trace();
            const size_t nr = (size_t)A * Nst, nm = (size_t)A * HU;
            HIP_CHECK(hipMemcpyAsync(t_rewards.p + nr * it, d_rewards.p, nr * 4, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(t_mean.p + nm * it, ps.gbest, nm * 4, hipMemcpyDeviceToDevice, stream));
            HIP_CHECK(hipMemcpyAsync(t_elites.p + (size_t)A * std::max(k, 1) * it, ps.gidx, (size_t)A * 4, hipMemcpyDeviceToDevice, stream));
        }
    }
    hipLaunchKernelGGL(k_take_first, dim3((A * U + 63) / 64), dim3(64), 0, stream, A, HU, U, ps.gbest, d_action.p);      // :114
    OptArgs oa = opt_args(step, 0u);
    for (int r = 0; r < shards_here; ++r) {
        if (ps_loopback > 1) oa.pop_offset = r * N;
        hipLaunchKernelGGL(k_pso_seed, dim3((N + 255) / 256, HU, A), dim3(256), 0, stream, oa, pso_state(r), d_var0.p, cfg.pso_v0_fraction, 0,
                           injected(BBMPC_NOISE_PSO_RESEED_TRUNC), injected(BBMPC_NOISE_PSO_RESEED_UNIFORM));          // :116-138
        HIP_CHECK(hipGetLastError());
    }
}

void Engine::evaluate_dev(const float* d_state_in, const float* d_seq, int n_pop, float* d_rew_out) {
    // rewards come back in the reference layout [n_pop, A]; the kernel writes [A][stride] so use a scratch
    // and a strided 2D copy (A is small).
    REQUIRE(n_pop >= 1, BBMPC_E_INVALID, "n_pop must be >= 1");
    if (particles_on()) {                                 // bbmpc_set_particles: the scores
        evaluate_particles_dev(d_state_in, d_seq, n_pop, d_rew_out, nullptr);
        return;
    }
    const int st = ((n_pop + 63) / 64) * 64;
    if (d_eval_rew.n < (size_t)A * st) d_eval_rew.alloc((size_t)A * st);
    RolloutArgs ra;
    memset(&ra, 0, sizeof(ra));
    ra.n_pop = n_pop; ra.A = A; ra.H = H; ra.U = U; ra.S = S; ra.HU = HU; ra.Nst = st;
    ra.agent_offset = cfg.agent_offset;
    ra.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
    ra.reward_kind = builtin_reward_kind();
    ra.state = d_state_in;
    ra.seq = d_seq;
    ra.lo = d_lo.p; ra.hi = d_hi.p;
    ra.rewards = d_eval_rew.p;
    launch_rollout(SRC_REF, false, ra);
    // [A][st] -> [n_pop][A]: per agent a strided copy (dst pitch A floats, width 1 float)
    for (int a = 0; a < A; ++a)
        HIP_CHECK(hipMemcpy2DAsync(d_rew_out + a, (size_t)A * 4, d_eval_rew.p + (size_t)a * st, 4, 4, n_pop,
                                   hipMemcpyDeviceToDevice, stream));
}

void Engine::step_dev(const float* d_states, const float* d_actions, int astride, int batch, float* d_next, float* d_rew) {
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    if (user_path() && (cfg.dynamics == BBMPC_DYN_USER || has_xform() || d_rew)) {
        // user dynamics / an inverse target transform, or a reward the built-in step kernels cannot evaluate: dynamics rows,
        // then reward rows
        float* nx = d_next;
        if (!nx) {
            if (u_next.n < (size_t)batch * S) u_next.alloc((size_t)batch * S);
            nx = u_next.p;
        }
        if (cfg.dynamics == BBMPC_DYN_USER || has_xform()) dynamics_rows(d_states, d_actions, astride, batch, nx);
        else step_dev(d_states, d_actions, astride, batch, nx, nullptr);
        if (d_rew) reward_rows(d_states, nx, d_actions, astride, batch, d_rew, 0);
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_MLP && batch <= 32 && !sw.mlp_generic) {
        // a handful of rows: one workgroup per row on plain FMAs -- the same per-row code as the control step's tail,
        // so act()'s predicted next state and evaluator.predict_next_state(obs, action) agree bit for bit
        REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
        hipLaunchKernelGGL(k_rows_mlp, dim3(batch), dim3(TAIL_THREADS), 0, stream, row_mlp(), S, U, builtin_reward_kind(),
                           (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER), d_states, d_actions, astride, d_next, d_rew);
        HIP_CHECK(hipGetLastError());
        return;
    }
    if (cfg.dynamics == BBMPC_DYN_MLP) {
        // one-step rollout of `batch` independent rows: per-particle start states, H = 1, actions as a
        // [batch,1,1,U] sequence
        const float* acts_c = dense_actions(d_actions, astride, batch);
        const int st_ = ((batch + 63) / 64) * 64;
        float* rew = d_rew;
        if (!rew) {
            if (d_step_c.n < (size_t)st_) d_step_c.alloc((size_t)st_);
            rew = d_step_c.p;
        }
        RolloutArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.n_pop = batch; ra.A = 1; ra.H = 1; ra.U = U; ra.S = S; ra.HU = U; ra.Nst = st_;
        ra.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER);
        ra.reward_kind = builtin_reward_kind();
        ra.state = d_states;
        ra.seq = acts_c;
        ra.lo = d_lo.p; ra.hi = d_hi.p;
        ra.rewards = rew;
        const bool prof = profiling;
        profiling = false;
        launch_rollout_mlp(SRC_REF, false, ra, true, d_next, nullptr);
        profiling = prof;
        return;
    }
    hipLaunchKernelGGL(k_step_pendulum, dim3((batch + 63) / 64), dim3(64), 0, stream, d_states, d_actions, astride, batch,
                       (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER), d_next, d_rew);
    HIP_CHECK(hipGetLastError());
}

void Engine::reward_dev(const float* d_cur, const float* d_next, const float* d_act, int batch, float* d_rew) {
    if (cfg.reward == BBMPC_REW_USER || cfg.reward == BBMPC_REW_MLP) {
        reward_rows(d_cur, d_next, d_act, U, batch, d_rew, 0);
        return;
    }
    hipLaunchKernelGGL(k_reward_only, dim3((batch + 63) / 64), dim3(64), 0, stream, d_cur, d_next, d_act, batch, S, U,
                       cfg.reward, (int)fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER), d_rew);
    HIP_CHECK(hipGetLastError());
}

// ------------------------------------------------------------------------------------------------
// parity hooks
// ------------------------------------------------------------------------------------------------
void Engine::inject(int kind, const float* data, int64_t count) {
    REQUIRE(auto_split <= 1 || !data, BBMPC_E_UNSUPPORTED, "injected noise is per shard: not available for a population > 32768 (played as shards)");
    if (!data) {
        inj.erase(kind);
        return;
    }
    switch (kind) {
        case BBMPC_NOISE_PSO_SCALARS: {
            REQUIRE(count == (int64_t)2 * std::max(iters, 1), BBMPC_E_INVALID, "PSO scalar noise must be [iters][2]");
            auto& b = inj[kind];
            b.alloc((size_t)count);
            HIP_CHECK(hipMemcpy(b.p, data, (size_t)count * 4, hipMemcpyHostToDevice));
            break;
        }
        case BBMPC_NOISE_TRUNC_NORMAL:
        case BBMPC_NOISE_UNIFORM:
        case BBMPC_NOISE_RADEMACHER:
        case BBMPC_NOISE_PSO_RESEED_TRUNC:
        case BBMPC_NOISE_PSO_RESEED_UNIFORM:
        case BBMPC_NOISE_PSO_RESET_POS:
        case BBMPC_NOISE_NORMAL:
        case BBMPC_NOISE_PSO_RESET_VEL: {
            const int nit = (kind == BBMPC_NOISE_TRUNC_NORMAL || kind == BBMPC_NOISE_RADEMACHER || kind == BBMPC_NOISE_NORMAL)
                                ? std::max(iters, 1) : 1;
            const int64_t per = (int64_t)N * A * HU;
            REQUIRE(count == per * nit, BBMPC_E_INVALID, "injected noise has the wrong element count");
            std::vector<float> tmp((size_t)A * HU * Nst * nit, 0.0f);
            for (int it = 0; it < nit; ++it) to_internal(data + per * it, N, tmp.data() + (size_t)A * HU * Nst * it);
            auto& b = inj[kind];
            b.alloc(tmp.size());
            HIP_CHECK(hipMemcpy(b.p, tmp.data(), tmp.size() * 4, hipMemcpyHostToDevice));
            break;
        }
        case BBMPC_NOISE_PROCESS: {
            REQUIRE(particles_on(), BBMPC_E_STATE, "process noise: call bbmpc_set_particles first (the layout depends on num_particles)");
            REQUIRE(count == (int64_t)A * part_P * H * S * std::max(iters, 1), BBMPC_E_INVALID, "process noise must be [iters][A,P,H,S]");
            auto& b = inj[kind];
            b.alloc((size_t)count);
            HIP_CHECK(hipMemcpy(b.p, data, (size_t)count * 4, hipMemcpyHostToDevice));
            break;
        }
        case BBMPC_NOISE_POLICY: {
            REQUIRE(prior_on(), BBMPC_E_STATE, "policy noise: call bbmpc_set_policy_prior_mlp first (the layout depends on count)");
            REQUIRE(count == (int64_t)A * prior_K * HU * std::max(iters, 1), BBMPC_E_INVALID, "policy noise must be [iters][A,K,H,U]");
            auto& b = inj[kind];
            b.alloc((size_t)count);
            HIP_CHECK(hipMemcpy(b.p, data, (size_t)count * 4, hipMemcpyHostToDevice));
            break;
        }
        case BBMPC_NOISE_EXPLORATION: {
            REQUIRE(count == (int64_t)A * U, BBMPC_E_INVALID, "exploration noise must be [A,U]");
            auto& b = inj[kind];
            b.alloc((size_t)count);
            HIP_CHECK(hipMemcpy(b.p, data, (size_t)count * 4, hipMemcpyHostToDevice));
            break;
        }
        default:
            throw HipError(BBMPC_E_UNSUPPORTED, "noise kind not supported yet");
    }
}

__global__ void k_dump_noise(RngKey key, uint32_t stream, uint32_t iter, int N, int A, int HU, int agent_offset,
                             float* out /* reference layout [N,A,HU] */) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * A * HU) return;
    const int j = idx % HU, a = (idx / HU) % A, n = idx / (HU * A);
    const U4 b = rng_block(key, stream, iter, (uint32_t)n, (uint32_t)(agent_offset + a), (uint32_t)j);
    const uint32_t w = pick_word(b, (uint32_t)j);
    float v;
    if (stream == BBMPC_NOISE_UNIFORM || stream == BBMPC_NOISE_PSO_RESEED_UNIFORM || stream == BBMPC_NOISE_PSO_RESET_POS ||
        stream == BBMPC_NOISE_PSO_RESET_VEL)
        v = word_to_uniform(w);
    else if (stream == BBMPC_NOISE_RADEMACHER)
        v = word_to_rademacher(w);
    else if (stream == BBMPC_NOISE_NORMAL)
        v = elem_normal(key, iter, n, agent_offset + a, j);
    else
        v = word_to_trunc_normal(w);
    out[idx] = v;
}

// the two scalar N(0,1) draws of PSO iteration `iter` (quirk Q3), same counter as pso_scalars (kernels_opt.hpp)
__global__ void k_dump_pso_scalars(OptArgs p, float* out) {
    float r1, r2;
    pso_scalars(p, nullptr, r1, r2);
    out[0] = r1;
    out[1] = r2;
}

void Engine::dump_noise(int kind, int control_step, int iteration, float* out, int64_t count) {
    int n = auto_split > 1 ? N * auto_split : N, a = A, hu = HU;       // (draws are keyed by the global particle)
    if (kind == BBMPC_NOISE_PROCESS) return dump_process_noise(control_step, iteration, out, count);
    if (kind == BBMPC_NOISE_POLICY) return dump_policy_noise(control_step, iteration, out, count);
    RngKey kk = key((uint32_t)control_step);
    if (kind == BBMPC_NOISE_PSO_SCALARS) {
        REQUIRE(count == 2, BBMPC_E_INVALID, "dump_noise: PSO scalars are [2] per (control step, iteration)");
        stage_read_back(*this, out, 2, [&](float* d) {
            hipLaunchKernelGGL(k_dump_pso_scalars, dim3(1), dim3(1), 0, stream, opt_args((uint32_t)control_step, (uint32_t)iteration), d);
        });
        return;
    }
    if (kind == BBMPC_NOISE_EXPLORATION) {
        n = 1; hu = U;
        kk.q_per_agent = (uint32_t)((U + 3) / 4);
    }
    const int64_t total = (int64_t)n * a * hu;
    REQUIRE(count == total, BBMPC_E_INVALID, "dump_noise: wrong element count");
    stage_read_back(*this, out, (size_t)total, [&](float* d) {
        hipLaunchKernelGGL(k_dump_noise, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, kk, (uint32_t)kind,
                           (uint32_t)iteration, n, a, hu, cfg.agent_offset, d);
    });
}

void Engine::get_trace(int it, int item, void* out, int64_t bytes) {
    REQUIRE(trace_on && t_rewards.p, BBMPC_E_STATE, "trace capture is not enabled or no optimize() call yet");
    REQUIRE(it >= 0 && it < std::max(iters, 1), BBMPC_E_INVALID, "trace iteration out of range");
    HIP_CHECK(hipStreamSynchronize(stream));
    const size_t nr = (size_t)A * Nst, nm = (size_t)A * HU, ns = (size_t)A * HU * Nst, ne = (size_t)A * std::max(k, 1);
    switch (item) {
        case BBMPC_TRACE_REWARDS: {
            const bool spsa = cfg.optimizer == BBMPC_OPT_SPSA;
            REQUIRE(bytes == (int64_t)N * A * 4 * (spsa ? 2 : 1), BBMPC_E_INVALID, "trace rewards: wrong size");
            std::vector<float> tmp(nr);
            float* o = (float*)out;
            for (int half = 0; half < (spsa ? 2 : 1); ++half) {
                HIP_CHECK(hipMemcpy(tmp.data(), (half ? t_rewards2.p : t_rewards.p) + nr * it, nr * 4, hipMemcpyDeviceToHost));
                for (int n = 0; n < N; ++n)
                    for (int a = 0; a < A; ++a) o[((size_t)half * N + n) * A + a] = tmp[(size_t)a * Nst + n];
            }
            break;
        }
        case BBMPC_TRACE_MEAN:
        case BBMPC_TRACE_VAR: {
            REQUIRE(bytes == (int64_t)nm * 4, BBMPC_E_INVALID, "trace mean/var: wrong size");
            HIP_CHECK(hipMemcpy(out, (item == BBMPC_TRACE_MEAN ? t_mean.p : t_var.p) + nm * it, nm * 4, hipMemcpyDeviceToHost));
            break;
        }
        case BBMPC_TRACE_ELITES: {
            const size_t cnt = (cfg.optimizer == BBMPC_OPT_CEM) ? (size_t)A * k
                               : (cfg.optimizer == BBMPC_OPT_CMAES ? (size_t)cma_G * k : (size_t)A);
            REQUIRE(bytes == (int64_t)cnt * 4, BBMPC_E_INVALID, "trace elites: wrong size");
            HIP_CHECK(hipMemcpy(out, t_elites.p + ne * it, cnt * 4, hipMemcpyDeviceToHost));
            break;
        }
        case BBMPC_TRACE_TOPK_PASSES: {
            REQUIRE(cfg.optimizer == BBMPC_OPT_CEM, BBMPC_E_INVALID, "trace top-k passes: CEM only");
            REQUIRE(bytes == (int64_t)A * 4, BBMPC_E_INVALID, "trace top-k passes: wrong size");
            HIP_CHECK(hipMemcpy(out, t_passes.p + (size_t)A * it, (size_t)A * 4, hipMemcpyDeviceToHost));
            break;
        }
        case BBMPC_TRACE_SAMPLES: {
            REQUIRE(bytes == (int64_t)N * A * HU * 4, BBMPC_E_INVALID, "trace samples: wrong size");
            std::vector<float> tmp(ns);
            HIP_CHECK(hipMemcpy(tmp.data(), t_samples.p + ns * it, ns * 4, hipMemcpyDeviceToHost));
            from_internal(tmp.data(), N, (float*)out);
            break;
        }
        case BBMPC_TRACE_CMA_SVD_STATS: {
            REQUIRE(cfg.optimizer == BBMPC_OPT_CMAES && t_cma_stats.p, BBMPC_E_STATE, "CMA-ES trace items need a traced CMA-ES control step");
            REQUIRE(bytes == (int64_t)cma_G * 16 * 4, BBMPC_E_INVALID, "CMA-ES SVD statistics: [G,16] int32");
            HIP_CHECK(hipMemcpy(out, t_cma_stats.p + (size_t)cma_G * 16 * it, (size_t)cma_G * 16 * 4, hipMemcpyDeviceToHost));
            break;
        }
        case BBMPC_TRACE_CMA_B:
        case BBMPC_TRACE_CMA_C:
        case BBMPC_TRACE_CMA_D: {
            REQUIRE(cfg.optimizer == BBMPC_OPT_CMAES && t_cma_B.p, BBMPC_E_STATE, "CMA-ES trace items need a traced CMA-ES control step");
            const size_t gn = (size_t)cma_G * cma_n, gnn = gn * cma_n;
            const size_t cnt = item == BBMPC_TRACE_CMA_D ? gn : gnn;
            REQUIRE(bytes == (int64_t)cnt * 4, BBMPC_E_INVALID, "CMA-ES trace item: wrong size");
            const float* src = item == BBMPC_TRACE_CMA_B ? t_cma_B.p : (item == BBMPC_TRACE_CMA_C ? t_cma_C.p : t_cma_D.p);
            HIP_CHECK(hipMemcpy(out, src + cnt * it, cnt * 4, hipMemcpyDeviceToHost));
            break;
        }
        default:
            throw HipError(BBMPC_E_INVALID, "unknown trace item");
    }
}

void Engine::get_state(const std::string& name, float* out, int64_t count) {
    HIP_CHECK(hipStreamSynchronize(stream));
    const size_t nm = (size_t)A * HU;
    const float* src = nullptr;
    if (name == "sample_buffer") {                            // the candidates as they lie in HBM, padding columns included: [A][HU][Nst]
        REQUIRE(d_samples.p, BBMPC_E_STATE, "this handle has no sample buffer");
        REQUIRE(count == (int64_t)A * HU * Nst, BBMPC_E_INVALID, "sample_buffer has A * H*U * Nst elements (Nst = population_size rounded up to 64)");
        HIP_CHECK(hipMemcpy(out, d_samples.p, (size_t)count * 4, hipMemcpyDeviceToHost));
        return;
    }
    if (constraint_raw_state(name, out, nullptr, count)) return;       // the chance constraint's buffers (bbmpc_particles.hip)
    if (name == "shaping_n_pop") {                            // candidates of the most recent shaped rollout (bbmpc_get_termination_steps' n / A); 0: none yet
        REQUIRE(count == 1, BBMPC_E_INVALID, "shaping_n_pop has one element");
        out[0] = (float)sh_last_npop;
        return;
    }
    if (cfg.optimizer == BBMPC_OPT_CMAES) goto cma_names;     // "sigma"/"m" etc. mean the CMA-ES state there
    if (name == "prev_mean") src = d_prev_mean.p;
    else if (name == "mean") src = d_mean.p;
    else if (name == "var") src = d_var.p;
    else if (name == "sigma") src = d_sigma.p;
cma_names:
    if (!src && cfg.optimizer == BBMPC_OPT_CMAES) {
        const size_t gn = (size_t)cma_G * cma_n, gnn = gn * cma_n;
        const float* v = nullptr;
        size_t cnt = gn;
        if (name == "m") v = c_m.p;
        else if (name == "sigma") v = c_sigma.p;
        else if (name == "p_sigma") v = c_ps.p;
        else if (name == "p_C") v = c_pc.p;
        else if (name == "D") v = c_Dd.p;
        else if (name == "C") { v = c_C.p; cnt = gnn; }
        else if (name == "B") { v = c_B.p; cnt = gnn; }
        REQUIRE(v, BBMPC_E_INVALID, "unknown state tensor '" + name + "'");
        REQUIRE(count == (int64_t)cnt, BBMPC_E_INVALID, "CMA-ES state tensor: wrong element count");
        HIP_CHECK(hipMemcpy(out, v, cnt * 4, hipMemcpyDeviceToHost));
        return;
    }
    if (!src && cfg.optimizer == BBMPC_OPT_PSO) {
        if (name == "pos" || name == "vel" || name == "pbest" || name == "pbest_r")
            REQUIRE(auto_split <= 1, BBMPC_E_UNSUPPORTED,      // (the loopback TEST hook keeps its documented meaning: shard 0's particles)
                    "per-particle state of a population_size > 32768 is kept per shard of the split: not available");
        const float* big = nullptr;
        if (name == "pos") big = d_cand_a.p;
        else if (name == "vel") big = d_vel.p;
        else if (name == "pbest") big = d_pbest.p;
        if (big) {            // [N,A,H,U] reference layout
            REQUIRE(count == (int64_t)N * A * HU, BBMPC_E_INVALID, "state tensor has N*A*H*U elements");
            std::vector<float> tmp((size_t)A * HU * Nst);
            HIP_CHECK(hipMemcpy(tmp.data(), big, tmp.size() * 4, hipMemcpyDeviceToHost));
            from_internal(tmp.data(), N, out);
            return;
        }
        if (name == "pbest_r") {
            REQUIRE(count == (int64_t)N * A, BBMPC_E_INVALID, "pbest_r has N*A elements");
            std::vector<float> tmp((size_t)A * Nst);
            HIP_CHECK(hipMemcpy(tmp.data(), d_pbest_r.p, tmp.size() * 4, hipMemcpyDeviceToHost));
            for (int n = 0; n < N; ++n)
                for (int a = 0; a < A; ++a) out[(size_t)n * A + a] = tmp[(size_t)a * Nst + n];
            return;
        }
        if (name == "gbest") src = d_gbest.p;
        if (name == "gbest_r") {
            REQUIRE(count == (int64_t)A, BBMPC_E_INVALID, "gbest_r has A elements");
            HIP_CHECK(hipMemcpy(out, d_gbest_r.p, (size_t)A * 4, hipMemcpyDeviceToHost));
            return;
        }
    }
    REQUIRE(src, BBMPC_E_INVALID, "unknown state tensor '" + name + "'");
    REQUIRE(count == (int64_t)nm, BBMPC_E_INVALID, "state tensor has A*H*U elements (C: G*n*n)");
    HIP_CHECK(hipMemcpy(out, src, nm * 4, hipMemcpyDeviceToHost));
}

void Engine::set_state(const std::string& name, const float* data, int64_t count) {
    HIP_CHECK(hipStreamSynchronize(stream));
    size_t nm = (size_t)A * HU;
    float* dst = nullptr;
    if (name == "sample_buffer") {                            // (tests: a sentinel in the padding columns)
        REQUIRE(d_samples.p, BBMPC_E_STATE, "this handle has no sample buffer");
        REQUIRE(count == (int64_t)A * HU * Nst, BBMPC_E_INVALID, "sample_buffer has A * H*U * Nst elements (Nst = population_size rounded up to 64)");
        HIP_CHECK(hipMemcpy(d_samples.p, data, (size_t)count * 4, hipMemcpyHostToDevice));
        return;
    }
    if (name != "constraint_shape" && constraint_raw_state(name, nullptr, data, count)) return;      // (tests: a sentinel in the padding)
    if (name == "prev_mean") dst = d_prev_mean.p;
    else if (name == "C" && cfg.optimizer == BBMPC_OPT_CMAES) { dst = c_C.p; nm = (size_t)cma_G * cma_n * cma_n; }   // (tests: a covariance at another scale)
    else if (name == "var0") { dst = d_var0.p; pi2_dist_ready = false; }
    cem_sigma0_ready = false;                  // (sigma0 follows prev_mean and var0)
    REQUIRE(dst, BBMPC_E_INVALID, "unknown/unsettable state tensor '" + name + "'");
    REQUIRE(count == (int64_t)nm, BBMPC_E_INVALID, "state tensor has A*H*U elements");
    HIP_CHECK(hipMemcpy(dst, data, nm * 4, hipMemcpyHostToDevice));
}

}  // namespace bbmpc

// ================================================================================================
// C ABI
// ================================================================================================
using bbmpc::Rccl;
using bbmpc::RecordComm;
using bbmpc::create_comm_stream;

extern "C" {

int bbmpc_abi_version(void) { return BBMPC_ABI_VERSION; }
const char* bbmpc_last_error(void) { return bbmpc::g_last_error.c_str(); }

int bbmpc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    int ok = 0;
    for (int i = 0; i < n; ++i) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strncmp(p.gcnArchName, "gfx950", 6) == 0) ++ok;
    }
    return ok;
}

int bbmpc_create(const bbmpc_config* cfg, bbmpc_handle* out) {
    API_BEGIN
    CHECK_PTR(cfg);
    CHECK_PTR(out);
    *out = nullptr;
    int caller_dev = -1;
    (void)hipGetDevice(&caller_dev);
    struct Restore {
        int d;
        ~Restore() { if (d >= 0) (void)hipSetDevice(d); }
    } restore{caller_dev};                       // the constructor selects cfg->device; the caller's device comes back
    Engine* e = new Engine(*cfg);
    *out = new bbmpc_handle_s{e};
    API_END
}

int bbmpc_destroy(bbmpc_handle h) {
    API_BEGIN
    if (h) {
        if (h->e) {
            DeviceGuard g(h->e->device);
            delete h->e;
        }
        delete h;
    }
    API_END
}

int bbmpc_set_stream(bbmpc_handle h, void* s) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(h->e->stream));
    h->e->stream = s ? (hipStream_t)s : h->e->own_stream;
    API_END
}

int bbmpc_set_stream_default(bbmpc_handle h) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(h->e->stream));
    h->e->stream = nullptr;
    API_END
}

int bbmpc_set_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* acts, const float* const* w,
                  const float* const* b, int32_t is_normalized, const float* const* stats) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->set_mlp(n_layers, dims, acts, w, b, is_normalized, stats);
    API_END
}

int bbmpc_set_mlp_ensemble(bbmpc_handle h, int32_t num_members, const float* const* w, const float* const* b) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_mlp_ensemble(num_members, w, b);
    API_END
}

int bbmpc_set_mlp_logvar_head(bbmpc_handle h, int32_t num_heads, const float* const* w, const float* const* b, const float* min_logvar,
                              const float* max_logvar) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_mlp_logvar_head(num_heads, w, b, min_logvar, max_logvar);
    API_END
}

// which = 0: process_input(states[B,S], actions[B,U]) -> [B,S+U];  1: process_output(states[B,S], raw[B,S]) -> [B,S]
static void process_io(Engine& e, int which, const float* a, const float* b, int batch, const float* const* stats, float* out) {
    if (batch < 1) throw HipError(BBMPC_E_INVALID, "batch must be >= 1");
    const int S = e.S, U = e.U;
    const size_t na = (size_t)batch * S, nb = (size_t)batch * (which == 0 ? U : S), no = (size_t)batch * (which == 0 ? S + U : S);
    const std::vector<float> flat = stats ? bbmpc::flatten_stats(stats, S, U) : std::vector<float>();     // (lives until finish())
    HostStage st(e);
    const int da = st.in(a, na), db = st.in(b, nb), dout = st.out(out, no), dst = st.in(flat.data(), flat.size());
    st.upload();
    if (which == 0) hipLaunchKernelGGL(bbmpc::k_process_input, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, e.stream, st[da], st[db], batch, S, U, st[dst], st[dout]);
    else hipLaunchKernelGGL(bbmpc::k_process_output, dim3((unsigned)((no + 255) / 256)), dim3(256), 0, e.stream, st[da], st[db], batch, S, U, st[dst], st[dout]);
    HIP_CHECK(hipGetLastError());
    st.finish();
}

int bbmpc_process_input(bbmpc_handle h, const float* states, const float* actions, int32_t batch, const float* const* stats, float* out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(actions);
    CHECK_PTR(out);
    process_io(*h->e, 0, states, actions, batch, stats, out);
    API_END
}

int bbmpc_process_output(bbmpc_handle h, const float* states, const float* raw_output, int32_t batch, const float* const* stats, float* out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(raw_output);
    CHECK_PTR(out);
    process_io(*h->e, 1, states, raw_output, batch, stats, out);
    API_END
}

int bbmpc_reset(bbmpc_handle h) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->reset();
    API_END
}

int bbmpc_optimize_dev(bbmpc_handle h, const float* d_state, int32_t, int32_t noise, float* d_record,
                       float* d_next_state) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    CHECK_PTR(d_state);
    CHECK_PTR(d_record);
    if (d_next_state == d_state) throw HipError(BBMPC_E_INVALID, "d_next_state must not alias d_state");
    h->e->optimize_dev(d_state, noise, d_record, d_next_state);
    API_END
}

}  // extern "C"

// ---- one host-in / host-out control step (bbmpc_optimize, bbmpc_optimize_gather): optimize_host and its parts ----
namespace bbmpc {

void Engine::ensure_completion_block() {
    if (host_done) return;
    HIP_CHECK(hipHostMalloc((void**)&host_done, (size_t)sync_lines() * 64, hipHostMallocCoherent | hipHostMallocMapped));   // engine.hpp: completion words | request lines | exit words
    memset(host_done, 0, (size_t)sync_lines() * 64);
    HIP_CHECK(hipHostGetDevicePointer((void**)&host_done_dev, host_done, 0));
    HIP_CHECK(hipMalloc((void**)&host_count, 8));
    HIP_CHECK(hipMemset(host_count, 0, 8));
}

void Engine::ensure_step_words() {
    if (step_words) return;
    HIP_CHECK(hipHostMalloc((void**)&step_words, 64, 0));        // staging for the (rare) re-synchronisation of the device words
    memset(step_words, 0, 64);
    HIP_CHECK(hipMalloc((void**)&step_words_dev, 64));
    HIP_CHECK(hipMemset(step_words_dev, 0, 64));
    step_mirror[0] = step_mirror[1] = 0xFFFFFFFFu;
}

// How a host-in / host-out control step travels: decided once per call from the handle's configuration, before anything
// is touched.
struct HostStepPlan {
    enum Transfer { kZeroCopyFused, kZeroCopyStaged, kCopies } transfer = kCopies;
    bool host_poll = false;     // the step's last kernel publishes a completion word (or line) that the host polls
    bool linger_ok = false;     // the resident form of the persistent pendulum kernel may serve / be launched
    bool stage = false;         // kZeroCopyStaged: the step's first kernel fetches the state from the pinned buffer itself
    bool graph_ok = false;      // kZeroCopyStaged: the step may be warmed up, captured and replayed as a graph
    uint64_t sig = 0;           // ... and what a graph of this call would have been captured for
};

static HostStepPlan choose_host_step(const Engine& e, int32_t noise) {
    HostStepPlan p;
    // single-kernel control steps read the state straight from the pinned, device-mapped host buffer; those and the
    // learned-dynamics path (whose last kernel, k_tail_mlp, owns the record) write the packed record straight into it
    const bool fused_step = e.sw.zero_copy && (e.use_fused() || e.use_fused_pso());   // PSO: the swarm re-seed that follows touches neither
    // every other optimizer path: the state goes to HBM once (many workgroups read it), the record comes back on its own --
    // whichever kernel packs it writes straight into the pinned buffer; k_tail_mlp, k_finalize_pendulum and the fused
    // CMA-ES kernel also publish the completion word, the rest is waited for on the stream
    const bool mlp_tail = e.sw.zero_copy && !fused_step && e.cfg.optimizer != BBMPC_OPT_NONE;
    if (!fused_step && !mlp_tail) return p;
    p.transfer = fused_step ? HostStepPlan::kZeroCopyFused : HostStepPlan::kZeroCopyStaged;
    // the last workgroup publishes a sequence number into a pinned host word right after the record stores
    // (publish_records_done): the call returns when the host sees it, ~10 us earlier than hipStreamSynchronize notices
    // the kernel's completion; the stream itself is joined lazily (settle)
    p.host_poll = e.sw.host_poll && !e.trace_on;
    // one agent on the persistent pendulum kernel: the previous call's kernel may still be there, waiting for this one
    p.linger_ok = fused_step && p.host_poll && e.sw.linger_us > 0 && e.A <= Engine::kLingerMaxAgents && e.use_fused() &&
                  !e.profiling && e.tail.event == nullptr &&
                  e.stream == e.own_stream;      // on a caller's stream it would hold back the caller's next work
    if (mlp_tail) {
        // hundreds of rollout workgroups read the state: it goes to HBM once, the record comes back on its own.
        // CEM / PI2 begin with k_dist_init, which fetches it from the pinned buffer itself; the others get a copy
        p.stage = (e.cfg.optimizer == BBMPC_OPT_CEM || e.cfg.optimizer == BBMPC_OPT_PI2) && !e.pop_sharded() &&
                  !e.user_path() && !e.value_on() && !e.shaping_on();
        // steady state of the learned-model PI2 / CEM path: the same launches with the same arguments every call --
        // replayed as a graph (engine.hpp: step_graph)
        p.graph_ok = e.sw.step_graph && p.stage && e.cfg.dynamics == BBMPC_DYN_MLP && p.host_poll &&
                     e.tail.event == nullptr && !e.profiling && !e.trace_on && !e.particles_on() && !e.corr_on() && !e.carry_on() && !e.prior_on() && !e.grad_on() && e.stream == e.own_stream && !e.any_injected();
        p.sig = ((uint64_t)e.mutations << 8) | (uint64_t)(noise ? 1 : 0) | 2u;
    }
    return p;
}

// Capture this call's launches as the handle's step graph; nothing runs until the graph is launched.  Returns whether
// there is a graph to replay now.
static bool capture_step_graph(Engine& e, const HostStepPlan& plan, int32_t noise, float* dpin, size_t ns) {
    if (e.step_graph) { (void)hipGraphExecDestroy(e.step_graph); e.step_graph = nullptr; }      // (captured for other arguments)
    e.ensure_step_words();
    const uint32_t saved_step = e.step_counter;
    hipGraph_t g = nullptr;
    bool ok = hipStreamBeginCapture(e.stream, hipStreamCaptureModeThreadLocal) == hipSuccess;
    if (ok) {
        ScopedRequest<const float*> staged(e.stage_state_src, dpin);
        e.step_capturing = true;
        try {
            e.optimize_dev(e.d_state.p, noise, dpin + ns, nullptr);
        } catch (...) { ok = false; }
        e.step_capturing = false;
        ok = (hipStreamEndCapture(e.stream, &g) == hipSuccess) && ok && g != nullptr && e.last_step_steady && e.stage_state_src == nullptr;
        if (ok) ok = hipGraphInstantiate(&e.step_graph, g, nullptr, nullptr, 0) == hipSuccess;
        if (g) (void)hipGraphDestroy(g);
    }
    e.step_counter = saved_step;                 // the captured call has not run
    (void)hipGetLastError();
    if (ok) {
        e.step_graph_sig = plan.sig;
        return true;
    }
    // this handle keeps enqueueing its launches one by one; why is kept (bbmpc_graph_stats' callers see 0 replays,
    // BBMPC_TRACE_GRAPH=1 prints it): a capture-illegal call added to the steady path must not go unnoticed
    e.step_graph = nullptr; e.sw.step_graph = 0;
    ++e.graph_capture_failures;
    if (getenv("BBMPC_TRACE_GRAPH")) fprintf(stderr, "[bbmpc] control-step graph capture / instantiate failed (steady=%d): replay disabled for this handle\n", (int)e.last_step_steady);
    return false;
}

static void replay_step_graph(Engine& e) {
    // the device's (control step, completion value) advance by themselves at the end of every replay; calls that
    // did not go through the graph in between put them out of step with the host's: one 8-byte copy then
    if (e.step_mirror[0] != e.step_counter || e.step_mirror[1] != e.host_seq) {
        HIP_CHECK(hipStreamSynchronize(e.stream));           // (the staging words may still be in use by an earlier copy)
        e.step_words[0] = e.step_counter; e.step_words[1] = e.host_seq;
        HIP_CHECK(hipMemcpyAsync(e.step_words_dev, e.step_words, 8, hipMemcpyHostToDevice, e.stream));
    }
    HIP_CHECK(hipGraphLaunch(e.step_graph, e.stream));
    ++e.calls_graph;
    ++e.step_counter;
    e.step_mirror[0] = e.step_counter;
    e.step_mirror[1] = e.host_seq + 1u == 0u ? 1u : e.host_seq + 1u;
    e.tail.attached = true;                      // the captured k_tail_mlp publishes the completion word
}

// after a step that was enqueued launch by launch: the run of consecutive eligible steady-state calls a capture waits for
static void count_warm_step(Engine& e, const HostStepPlan& plan) {
    if (plan.graph_ok && e.last_step_steady && e.step_warm_sig == plan.sig) ++e.step_graph_warm;
    else { e.step_graph_warm = (plan.graph_ok && e.last_step_steady) ? 1 : 0; e.step_warm_sig = plan.sig; }
}

// kZeroCopyStaged: replay, capture and replay, or enqueue the step's launches one by one
static void run_staged_step(Engine& e, const HostStepPlan& plan, int32_t noise, const float* pin, float* dpin, size_t ns) {
    const bool replay = plan.graph_ok && ((e.step_graph && e.step_graph_sig == plan.sig) ||
                                          (e.step_graph_warm >= 3 && e.step_warm_sig == plan.sig && capture_step_graph(e, plan, noise, dpin, ns)));
    if (replay) {
        replay_step_graph(e);
        return;
    }
    {
        ScopedRequest<const float*> staged(e.stage_state_src, plan.stage ? dpin : nullptr);
        if (!plan.stage) HIP_CHECK(hipMemcpyAsync(e.d_state.p, pin, ns * 4, hipMemcpyHostToDevice, e.stream));
        e.optimize_dev(e.d_state.p, noise, dpin + ns, nullptr);
        if (e.stage_state_src) throw HipError(BBMPC_E_HIP, "internal: the control step did not stage its state");
    }
    count_warm_step(e, plan);
}

enum class RecordWait { kServed, kPublished, kStream };   // the record is here | announced by the step's last kernel | behind the stream

// The zero-copy forms: the step's kernels read the [A,S] state and write the packed record straight from / to the
// pinned, device-mapped host buffer (a few PCIe transactions) -- no copy-engine round trips around a ~50 us kernel.
static RecordWait run_zero_copy_step(Engine& e, const HostStepPlan& plan, int32_t noise, float* pin, size_t ns) {
    float* dpin = e.h_pin_dev;
    if (plan.host_poll) {
        e.ensure_completion_block();
        if (++e.host_seq == 0) e.host_seq = 1;
    }
    bool handled = false;                // served by the resident workgroups: the records are already in the pinned buffer
    if (e.resident_alive) {
        if (plan.linger_ok) handled = e.resident_step(pin, noise, e.host_seq, pin + ns);
        else e.resident_stop();
    }
    if (handled) {
        ++e.calls_resident;
        return RecordWait::kServed;
    }
    ++e.calls_launched;
    ClearOnThrow<int> subset(e.subset_n);                   // a subset named by resident_step must not outlive the call it was for
    TailRequest want(e, plan.host_poll ? e.host_done_dev : nullptr, e.host_count, e.host_seq);
    ScopedRequest<bool> linger(e.linger_launch, plan.linger_ok && e.subset_n == 0);      // a subset launch (after a crossed exit) is an ordinary one
    if (plan.transfer == HostStepPlan::kZeroCopyFused) e.optimize_dev(dpin, noise, dpin + ns, nullptr);
    else run_staged_step(e, plan, noise, pin, dpin, ns);
    subset.done();
    return want.taken() ? RecordWait::kPublished : RecordWait::kStream;
}

static void run_copied_step(Engine& e, int32_t noise, float* pin, size_t ns, size_t nr) {
    ++e.calls_launched;
    HIP_CHECK(hipMemcpyAsync(e.d_state.p, pin, ns * 4, hipMemcpyHostToDevice, e.stream));
    e.optimize_dev(e.d_state.p, noise, e.d_record.p, nullptr);
    HIP_CHECK(hipMemcpyAsync(pin + ns, e.d_record.p, nr * 4, hipMemcpyDeviceToHost, e.stream));
}

static void wait_for_records(Engine& e, RecordWait how, float* records) {
    if (how == RecordWait::kStream) {
        HIP_CHECK(hipStreamSynchronize(e.stream));
        e.lazy_sync = false;
        return;
    }
    if (how == RecordWait::kPublished) {
        const uint32_t want = e.host_seq;
        const auto t0 = std::chrono::steady_clock::now();
        const auto unpublished = [] { return HipError(BBMPC_E_HIP, "bbmpc_optimize: the control step finished without publishing its records"); };
        if (e.resident_alive) {
            // a LINGER launch: every agent's workgroup publishes its own completion line, which carries the record
            for (int a = 0; a < e.A; ++a) {
                volatile const uint32_t* f = e.ack_host(a);
                float* rec_a = records + (size_t)a * kCompletionRecordFloats;
                spin_until(t0, [&] { return completion_line_decode(f, want, rec_a); }, [&] {
                    e.resident_stop();                               // a fault surfaces in its synchronize
                    if (!completion_line_decode(f, want, rec_a)) throw unpublished();
                    return true;
                });
            }
        } else {
            volatile const uint32_t* f = e.host_done;
            spin_until(t0, [&] { return *f == want; }, [&] {
                HIP_CHECK(hipStreamSynchronize(e.stream));       // a fault surfaces here; otherwise the word must be there
                if (*f != want) throw unpublished();
                return true;
            });
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    e.lazy_sync = true;
}

static void unpack_records(const Engine& e, const float* r, float* action, float* next_state, float* reward) {
    for (int a = 0; a < e.A; ++a) {
        if (action) memcpy(action + (size_t)a * e.U, r + (size_t)a * e.rec, e.U * 4);
        if (next_state) memcpy(next_state + (size_t)a * e.S, r + (size_t)a * e.rec + e.U, e.S * 4);
        if (reward) reward[a] = r[(size_t)a * e.rec + e.U + e.S];
    }
}

}  // namespace bbmpc

// One host-in / host-out control step (the body of bbmpc_optimize, shared with bbmpc_optimize_gather): returns the packed
// records [A][U+S+1] in the handle's pinned buffer.  The caller has NOT settled the handle: consecutive calls are ordered
// by the stream (or served by the resident kernel), everything else settles first.
static const float* optimize_host(bbmpc::Engine& e, const float* state, int32_t noise, float* action, float* next_state, float* reward) {
    using namespace bbmpc;
    const size_t ns = (size_t)e.A * e.S, nr = (size_t)e.A * e.rec;
    float* pin = e.pinned(ns + nr);
    memcpy(pin, state, ns * 4);
    const HostStepPlan plan = choose_host_step(e, noise);
    RecordWait how = RecordWait::kStream;
    if (plan.transfer == HostStepPlan::kCopies) run_copied_step(e, noise, pin, ns, nr);
    else how = run_zero_copy_step(e, plan, noise, pin, ns);
    e.note_in_flight();                  // launch path: the kernels are enqueued
    wait_for_records(e, how, pin + ns);
    unpack_records(e, pin + ns, action, next_state, reward);
    return pin + ns;
}

extern "C" {

int bbmpc_optimize(bbmpc_handle h, const float* state, int32_t t, int32_t noise, float* action, float* next_state,
                   float* reward) {
    API_BEGIN
    CHECK_HANDLE_NOSETTLE(h);            // consecutive calls are ordered by the stream; everything else settles first
    CHECK_PTR(state);
    (void)t;  // the reference evaluator accepts and ignores time_step (deterministic.py:26)
    (void)optimize_host(*h->e, state, noise, action, next_state, reward);
    API_END
}

int bbmpc_rollout_episode(bbmpc_handle h, const float* start_state, int32_t num_steps, int32_t noise, float* records_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    CHECK_PTR(start_state);
    CHECK_PTR(records_out);
    Engine& e = *h->e;
    if (num_steps < 1) throw HipError(BBMPC_E_INVALID, "num_steps must be >= 1");
    const size_t ns = (size_t)e.A * e.S, nr = (size_t)e.A * e.rec;
    HostStage st(e);
    const int s0 = st.in(start_state, ns), s1 = st.scratch(ns), r = st.out(records_out, nr * (size_t)num_steps);
    st.upload();
    float* const state[2] = {st[s0], st[s1]};                                // the state ping-pong
    for (int t = 0; t < num_steps; ++t) e.optimize_dev(state[t & 1], noise, st[r] + nr * t, state[(t + 1) & 1]);
    st.finish();
    API_END
}

int bbmpc_evaluate_dev(bbmpc_handle h, const float* d_state, const float* d_seq, int32_t n_pop, float* d_rewards) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_state);
    CHECK_PTR(d_seq);
    CHECK_PTR(d_rewards);
    h->e->evaluate_dev(d_state, d_seq, n_pop, d_rewards);
    API_END
}

int bbmpc_evaluate(bbmpc_handle h, const float* state, const float* seq, int32_t n_pop, float* rewards) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(state);
    CHECK_PTR(seq);
    CHECK_PTR(rewards);
    Engine& e = *h->e;
    if (n_pop < 1) throw HipError(BBMPC_E_INVALID, "n_pop must be >= 1");
    HostStage st(e);
    const int q = st.in(seq, (size_t)n_pop * e.A * e.HU), r = st.out(rewards, (size_t)n_pop * e.A);
    st.upload();
    HIP_CHECK(hipMemcpyAsync(e.d_state.p, state, (size_t)e.A * e.S * 4, hipMemcpyHostToDevice, e.stream));   // (not a slot: DESIGN.md section 3a)
    e.evaluate_dev(e.d_state.p, st[q], n_pop, st[r]);
    st.finish();
    API_END
}

int bbmpc_step_dev(bbmpc_handle h, const float* d_states, const float* d_actions, int32_t astride, int32_t batch,
                   float* d_next, float* d_rew) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_actions);
    h->e->step_dev(d_states, d_actions, astride, batch, d_next, d_rew);
    API_END
}

int bbmpc_predict_next_state(bbmpc_handle h, const float* states, const float* actions, int32_t batch, float* next) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(actions);
    CHECK_PTR(next);
    Engine& e = *h->e;
    if (batch < 1) throw HipError(BBMPC_E_INVALID, "batch must be >= 1");
    HostStage st(e);
    const int s = st.in(states, (size_t)batch * e.S), a = st.in(actions, (size_t)batch * e.U), n = st.out(next, (size_t)batch * e.S);
    st.upload();
    e.step_dev(st[s], st[a], e.U, batch, st[n], nullptr);
    st.finish();
    API_END
}

int bbmpc_evaluate_next_reward(bbmpc_handle h, const float* states, const float* next_states, const float* actions,
                               int32_t batch, float* rewards) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(next_states);
    CHECK_PTR(actions);
    CHECK_PTR(rewards);
    Engine& e = *h->e;
    if (batch < 1) throw HipError(BBMPC_E_INVALID, "batch must be >= 1");
    HostStage st(e);
    const int c = st.in(states, (size_t)batch * e.S), n = st.in(next_states, (size_t)batch * e.S);
    const int a = st.in(actions, (size_t)batch * e.U), r = st.out(rewards, (size_t)batch);
    st.upload();
    e.reward_dev(st[c], st[n], st[a], batch, st[r]);
    st.finish();
    API_END
}

int bbmpc_inject_noise(bbmpc_handle h, int32_t kind, const float* data, int64_t count) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(h->e->stream));
    h->e->inject(kind, data, count);
    API_END
}

int bbmpc_dump_noise(bbmpc_handle h, int32_t kind, int32_t control_step, int32_t iteration, float* out, int64_t count) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(out);
    h->e->dump_noise(kind, control_step, iteration, out, count);
    API_END
}

int bbmpc_set_trace(bbmpc_handle h, int32_t enabled) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    if (enabled && h->e->auto_split > 1)
        throw HipError(BBMPC_E_UNSUPPORTED, "the parity trace is per shard: not available for a population > 32768 (played as shards)");
    h->e->trace_on = enabled != 0;
    API_END
}

int bbmpc_set_sampling_correlation(bbmpc_handle h, const float* mix, int64_t count) {
    API_BEGIN
    CHECK_HANDLE(h);                     // (settles the handle: a resident control-step kernel is stopped first)
    h->e->set_sampling_correlation(mix, count);
    API_END
}

int bbmpc_get_sampling_correlation(bbmpc_handle h, int32_t* installed) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(installed);
    *installed = h->e->corr_on() ? 1 : 0;
    API_END
}

int bbmpc_set_elite_carry(bbmpc_handle h, int keep, int shift) {
    API_BEGIN
    CHECK_HANDLE(h);                     // (settles the handle: a resident control-step kernel is stopped first)
    h->e->set_elite_carry(keep, shift);
    API_END
}

int bbmpc_get_elite_carry(bbmpc_handle h, int* keep, int* shift, int* stored) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(keep);
    CHECK_PTR(shift);
    CHECK_PTR(stored);
    *keep = h->e->carry_keep;
    *shift = h->e->carry_shift;
    *stored = h->e->carry_stored;
    API_END
}

int bbmpc_get_trace(bbmpc_handle h, int32_t iteration, int32_t item, void* out, int64_t bytes) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(out);
    h->e->get_trace(iteration, item, out, bytes);
    API_END
}

int bbmpc_get_state(bbmpc_handle h, const char* name, float* out, int64_t count) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(name);
    CHECK_PTR(out);
    h->e->get_state(name, out, count);
    API_END
}

int bbmpc_set_state(bbmpc_handle h, const char* name, const float* data, int64_t count) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    CHECK_PTR(name);
    CHECK_PTR(data);
    h->e->set_state(name, data, count);
    API_END
}

int bbmpc_set_profiling(bbmpc_handle h, int32_t enabled) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->profiling = enabled != 0;
    h->e->prof_every = enabled > 1 ? enabled : 1;
    h->e->prof_seq = 0;
    API_END
}

int bbmpc_get_profile(bbmpc_handle h, double* ms, int64_t* launches, const char** name) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(ms);
    CHECK_PTR(launches);
    h->e->get_profile(ms, launches);
    if (name) *name = h->e->dominant_kernel;
    API_END
}

int bbmpc_profile_instantiation(bbmpc_handle h, const char** name) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(name);
    const Engine& e = *h->e;
    // the recorded instantiation belongs to the dominant kernel only while that kernel is the one being launched
    const size_t nb = strlen(e.dominant_kernel);
    *name = (e.dominant_inst[0] && strncmp(e.dominant_inst, e.dominant_kernel, nb) == 0 && e.dominant_inst[nb] == '<') ? e.dominant_inst
                                                                                                                    : e.dominant_kernel;
    API_END
}

int bbmpc_synchronize(bbmpc_handle h) {
    API_BEGIN
    CHECK_HANDLE(h);
    HIP_CHECK(hipStreamSynchronize(h->e->stream));
    if (h->e->rc.stream) HIP_CHECK(hipStreamSynchronize(h->e->rc.stream));
    API_END
}

int bbmpc_comm_unique_id(void* out, int64_t bytes) {
    API_BEGIN
    CHECK_PTR(out);
    if (bytes < (int64_t)sizeof(Rccl::UniqueId)) throw HipError(BBMPC_E_INVALID, "bbmpc_comm_unique_id: buffer smaller than BBMPC_COMM_ID_BYTES");
    const Rccl& r = Rccl::get();
    Rccl::UniqueId id;
    r.check(r.GetUniqueId(&id), "ncclGetUniqueId");
    memcpy(out, &id, sizeof(id));
    API_END
}

// stream, events and hand-off flags of a handle's communicator, whoever serves it (`join` creates c.comm)
static void comm_setup(Engine* e, int32_t nranks, int32_t rank, const Rccl& api, const char* what, const std::function<int(Rccl::Comm*)>& join) {
    if (nranks < 1 || rank < 0 || rank >= nranks) throw HipError(BBMPC_E_INVALID, "bbmpc_comm_init: rank / nranks out of range");
    if (e->rc.comm) throw HipError(BBMPC_E_STATE, "bbmpc_comm_init: the handle already has a communicator");
    RecordComm& c = e->rc;
    c.stream = create_comm_stream();
    for (int s = 0; s < RecordComm::kSlots; ++s) {
        HIP_CHECK(hipEventCreateWithFlags(&c.ready[s], hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&c.done[s], hipEventDisableTiming));
    }
    const int irc = join(&c.comm);
    if (irc != 0) {
        c.comm = nullptr;
        c.destroy();                     // stream + events created above
        api.check(irc, what);
    }
    c.api = &api;
    c.nranks = nranks;
    c.rank = rank;
    // BBMPC_COMM_SYNC=event: events only; default: flags in signal memory where the device supports stream wait-value
    int can_wait = 0;
    (void)hipDeviceGetAttribute(&can_wait, hipDeviceAttributeCanUseStreamWaitValue, e->device);
    const char* sm = getenv("BBMPC_COMM_SYNC");
    c.sync_mode = can_wait ? 1 : 0;
    if (sm && !strcmp(sm, "event")) c.sync_mode = 0;
    if (c.sync_mode != 0) {
        // signal memory comes in 8-byte units, lives in host memory and can be polled by the host
        bool ok = hipExtMallocWithFlags((void**)&c.flag, 8, hipMallocSignalMemory) == hipSuccess;
        for (int s = 0; ok && s < RecordComm::kSlots; ++s)
            ok = hipExtMallocWithFlags((void**)&c.done_flag[s], 8, hipMallocSignalMemory) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            c.sync_mode = 0;
        } else {
            HIP_CHECK(hipMalloc((void**)&c.count, 8));
            HIP_CHECK(hipMemset(c.count, 0, 8));
            HIP_CHECK(hipMemset(c.flag, 0, 8));
            for (int s = 0; s < RecordComm::kSlots; ++s) HIP_CHECK(hipMemset(c.done_flag[s], 0, 8));
            // test hook: start the sequence numbers just below the wrap (tests/test_gpu_comm.py)
            if (const char* s0 = getenv("BBMPC_COMM_SEQ_START")) {
                c.seq = (uint32_t)strtoul(s0, nullptr, 0);
                HIP_CHECK(hipMemcpy(c.flag, &c.seq, 4, hipMemcpyHostToDevice));
                for (int s = 0; s < RecordComm::kSlots; ++s) {
                    HIP_CHECK(hipMemcpy(c.done_flag[s], &c.seq, 4, hipMemcpyHostToDevice));
                    c.done_seq[s] = c.seq;
                }
            }
        }
    }
}

int bbmpc_comm_init(bbmpc_handle h, const void* unique_id, int32_t nranks, int32_t rank) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    CHECK_PTR(unique_id);
    const Rccl& r = Rccl::get();            // (the handle's device is current: CHECK_HANDLE)
    Rccl::UniqueId id;
    memcpy(&id, unique_id, sizeof(id));
    comm_setup(h->e, nranks, rank, r, "ncclCommInitRank", [&](Rccl::Comm* out) { return r.CommInitRank(out, nranks, id, rank); });
    API_END
}

int bbmpc_comm_init_local(bbmpc_handle h, uint64_t group_key, int32_t nranks, int32_t rank) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    Engine* e = h->e;
    comm_setup(e, nranks, rank, Rccl::local(), "bbmpc_comm_init_local",
               [&](Rccl::Comm* out) { return bbmpc::local_comm_join(group_key, nranks, rank, e->device, out); });
    API_END
}

// sequence number of the next hand-off (flag modes)
static uint32_t next_comm_seq(Engine* e) {
    RecordComm& c = e->rc;
    if (c.seq >= 0x7fffffffu) {                                        // wrap: once per 2^31 control steps
        HIP_CHECK(hipStreamSynchronize(e->stream));
        HIP_CHECK(hipStreamSynchronize(c.stream));
        HIP_CHECK(hipMemset(c.flag, 0, 8));
        for (int s = 0; s < RecordComm::kSlots; ++s) {
            HIP_CHECK(hipMemset(c.done_flag[s], 0, 8));
            c.done_seq[s] = 0;
            c.pending[s] = false;
        }
        c.seq = 0;
    }
    return ++c.seq;
}

// Enqueue the all-gather of `count` floats per rank behind everything the launch stream holds so far.
//
// Hand-off launch stream -> communication stream, two forms:
//  * `published`: the control step was one persistent kernel and its last workgroup publishes sequence number `v` in
//    signal memory (kernels_fused.hpp); the communication stream waits for the value.  Nothing is added to the
//    launch stream: +2 us per control step against no gather at all (tools/gather_overhead.py).
//  * otherwise an event (`event_attached`: it already rides on the last kernel's dispatch packet).  A cross-stream
//    event costs the launch stream 5-9 us per control step -- the runtime adds a barrier packet and a completion
//    signal between two back-to-back kernels -- which only matters for ~50 us control steps, and those are the
//    single-kernel ones.  (A wait-value that sits in the queue across many launches is worse: the command processor
//    polls it between the other queue's dispatches; measured +77 us on a 25-launch control step.)
// Completion (sync_mode 1) goes to a second flag that the host polls in bbmpc_gather_wait: an event recorded on the
// communication stream and queried from the host was measured to cost the launch stream another 4 us per step.
// the collective itself + "slot done" on the communication stream (whatever made d_records ready is already ordered before it there)
static void gather_enqueue(Engine* e, const float* d_records, float* d_gathered, size_t count, int slot, uint32_t v) {
    RecordComm& c = e->rc;
    const Rccl& r = *c.api;
    r.check(r.AllGather(d_records, d_gathered, count, Rccl::kFloat32, c.comm, c.stream), "ncclAllGather");
    if (c.sync_mode == 1) {
        HIP_CHECK(hipStreamWriteValue32(c.stream, c.done_flag[slot], v, 0));
        c.done_seq[slot] = v;
    } else {
        HIP_CHECK(hipEventRecord(c.done[slot], c.stream));
    }
    c.pending[slot] = true;
}

// staged records of earlier bbmpc_optimize_gather calls -> HBM -> collective, on the communication stream
static void flush_deferred_gathers(Engine* e) {
    RecordComm& c = e->rc;
    if (!c.comm) return;
    const size_t nr = (size_t)e->A * e->rec;
    for (int s = 0; s < RecordComm::kSlots; ++s) {
        if (!e->gather_deferred[s]) continue;
        e->gather_deferred[s] = false;
        HIP_CHECK(hipMemcpyAsync(e->d_record_slot[s].p, e->h_record_stage[s], nr * sizeof(float), hipMemcpyHostToDevice, c.stream));
        gather_enqueue(e, e->d_record_slot[s].p, e->gather_deferred_dst[s], nr, s, c.sync_mode == 1 ? next_comm_seq(e) : 0u);
    }
}

static void gather_records(Engine* e, const float* d_records, float* d_gathered, size_t count, int slot, bool event_attached,
                           bool published, uint32_t v) {
    RecordComm& c = e->rc;
    if (published) {
        HIP_CHECK(hipStreamWaitValue32(c.stream, c.flag, v, hipStreamWaitValueGte, 0xffffffffu));
    } else {
        if (!event_attached) HIP_CHECK(hipEventRecord(c.ready[slot], e->stream));
        HIP_CHECK(hipStreamWaitEvent(c.stream, c.ready[slot], 0));
    }
    gather_enqueue(e, d_records, d_gathered, count, slot, v);
}

// The first check of every gather entry point (in front of its pointer checks).
// The communicator of a population-sharded handle carries the per-iteration partials on the LAUNCH stream; one RCCL
// communicator must not be driven from two unsynchronised streams, so such a handle has no record gather (its ranks
// all hold the same agents: there is nothing to gather).  A population that is only split into shards on THIS GPU
// (population_size > 32768, or the loopback hook) never drives the communicator and gathers like any other handle
static void refuse_gather_when_sharded_over_ranks(const Engine* e) {
    if (e->pop_sharded_across_ranks()) throw HipError(BBMPC_E_UNSUPPORTED, "record gather on a handle whose population is sharded over ranks (every rank already holds every agent's record)");
}

// ... and the last ones (behind them): the handle's communicator, with `slot` free for entry point `who` to use.
// count: bbmpc_gather_records_dev's own argument, checked where that entry point always checked it.
static RecordComm& gather_comm(Engine* e, const char* who, int32_t slot, const int64_t* count = nullptr) {
    RecordComm& c = e->rc;
    const auto refusal = [who](int code, const char* why) { return HipError(code, std::string(who) + why); };
    if (!c.comm) throw refusal(BBMPC_E_STATE, ": call bbmpc_comm_init first");
    if (slot < 0 || slot >= RecordComm::kSlots) throw refusal(BBMPC_E_INVALID, ": slot must be 0 or 1");
    if (count && *count <= 0) throw refusal(BBMPC_E_INVALID, ": count must be positive");
    if (c.pending[slot]) throw refusal(BBMPC_E_STATE, ": slot still pending (call bbmpc_gather_wait)");
    return c;
}

int bbmpc_gather_records_dev(bbmpc_handle h, const float* d_records, float* d_gathered, int64_t count, int32_t slot) {
    API_BEGIN
    CHECK_HANDLE(h);
    Engine* e = h->e;
    refuse_gather_when_sharded_over_ranks(e);
    CHECK_PTR(d_records);
    CHECK_PTR(d_gathered);
    RecordComm& c = gather_comm(e, "bbmpc_gather_records_dev", slot, &count);
    gather_records(e, d_records, d_gathered, (size_t)count, slot, false, false, c.sync_mode ? next_comm_seq(e) : 0u);
    API_END
}

int bbmpc_optimize_gather_dev(bbmpc_handle h, const float* d_state, int32_t, int32_t noise, float* d_records,
                              float* d_next_state, float* d_gathered, int32_t slot) {
    API_BEGIN
    CHECK_HANDLE(h);
    Engine* e = h->e;
    e->invalidate_step_graph();
    refuse_gather_when_sharded_over_ranks(e);
    CHECK_PTR(d_state);
    CHECK_PTR(d_records);
    CHECK_PTR(d_gathered);
    if (d_next_state == d_state) throw HipError(BBMPC_E_INVALID, "d_next_state must not alias d_state");
    RecordComm& c = gather_comm(e, "bbmpc_optimize_gather_dev", slot);
    // single-launch control steps carry the hand-off themselves: the sequence number published by the kernel's last
    // workgroup, or (BBMPC_COMM_SYNC=event) the ready event on the kernel's dispatch packet
    const uint32_t v = c.sync_mode == 1 ? next_comm_seq(e) : 0u;
    bool taken = false;
    {
        using bbmpc::TailRequest;
        const TailRequest want = c.sync_mode == 1 ? TailRequest(*e, c.flag, c.count, v) : TailRequest(*e, c.ready[slot]);
        e->optimize_dev(d_state, noise, d_records, d_next_state);
        taken = want.taken();
    }
    gather_records(e, d_records, d_gathered, (size_t)e->A * e->rec, slot, c.sync_mode == 0 && taken, c.sync_mode == 1 && taken, v);
    API_END
}

// MPCPolicy.act of one rank of an agent-sharded run: host state in, host action / next state / reward out for the
// LOCAL agents (synchronous), plus the all-gather of their records enqueued on the communication stream, where it
// overlaps the caller's next control step (bbmpc_gather_wait(slot) before the slot is reused).
int bbmpc_optimize_gather(bbmpc_handle h, const float* state, int32_t, int32_t noise, float* action, float* next_state,
                          float* reward, float* d_gathered, int32_t slot) {
    API_BEGIN
    CHECK_HANDLE_NOSETTLE(h);            // as bbmpc_optimize: consecutive calls are ordered by the stream / the resident kernel
    Engine* e = h->e;
    e->invalidate_step_graph();
    refuse_gather_when_sharded_over_ranks(e);
    CHECK_PTR(state);
    CHECK_PTR(d_gathered);
    RecordComm& c = gather_comm(e, "bbmpc_optimize_gather", slot);
    // this rank's agents: exactly bbmpc_optimize (zero-copy state, records polled from pinned memory, resident kernel).
    // While the control step runs on the GPU the host enqueues the collective of the PREVIOUS call's records: the
    // ~20 us of host API time (H2D copy, ncclAllGather, completion word) hide under the kernel instead of sitting
    // between two control steps.  This call's own records are staged at the end and travel during the next call, or
    // when anything settles the handle (bbmpc_gather_wait on the slot, bbmpc_synchronize, any other entry point).
    const size_t nr = (size_t)e->A * e->rec;
    if (!e->d_record_slot[slot].p) e->d_record_slot[slot].alloc(nr);
    if (!e->h_record_stage[slot])
        HIP_CHECK(hipHostMalloc((void**)&e->h_record_stage[slot], nr * sizeof(float), hipHostMallocDefault));
    const float* rec = nullptr;
    {
        e->in_flight_called = false;
        bbmpc::ScopedRequest<void (*)(Engine*)> hook(e->in_flight_hook, flush_deferred_gathers);
        rec = optimize_host(*e, state, noise, action, next_state, reward);
    }
    if (!e->in_flight_called) flush_deferred_gathers(e);
    memcpy(e->h_record_stage[slot], rec, nr * sizeof(float));      // the slot is free: its last gather was waited for (pending == false)
    e->gather_deferred[slot] = true;
    e->gather_deferred_dst[slot] = d_gathered;
    e->settle_hook = flush_deferred_gathers;
    c.pending[slot] = true;
    API_END
}

int bbmpc_call_stats(bbmpc_handle h, int64_t* served_resident, int64_t* launched) {
    API_BEGIN
    CHECK_HANDLE(h);
    if (served_resident) *served_resident = h->e->calls_resident;
    if (launched) *launched = h->e->calls_launched;
    API_END
}

int bbmpc_graph_stats(bbmpc_handle h, int64_t* replayed) {
    API_BEGIN
    CHECK_HANDLE(h);
    if (replayed) *replayed = h->e->calls_graph;
    API_END
}

int bbmpc_handle_device(bbmpc_handle h, int32_t* device) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(device);
    *device = h->e->device;
    API_END
}

// What the communicator itself reports (ncclCommCount / ncclCommUserRank) + the hand-off mode in use:
// sync_mode 1 = sequence numbers in signal memory, 0 = events.
int bbmpc_comm_info(bbmpc_handle h, int32_t* nranks, int32_t* rank, int32_t* sync_mode) {
    API_BEGIN
    CHECK_HANDLE(h);
    RecordComm& c = h->e->rc;
    if (!c.comm) throw HipError(BBMPC_E_STATE, "bbmpc_comm_info: no communicator (bbmpc_comm_init)");
    const Rccl& r = *c.api;
    int n = 0, me = 0;
    r.check(r.CommCount(c.comm, &n), "ncclCommCount");
    r.check(r.CommUserRank(c.comm, &me), "ncclCommUserRank");
    if (nranks) *nranks = n;
    if (rank) *rank = me;
    if (sync_mode) *sync_mode = c.sync_mode;
    API_END
}

int bbmpc_gather_wait(bbmpc_handle h, int32_t slot, int32_t host_block) {
    API_BEGIN
    CHECK_HANDLE_NOSETTLE(h);            // part of the control loop: must not stop a resident kernel
    Engine* e = h->e;
    RecordComm& c = e->rc;
    if (slot < 0 || slot >= RecordComm::kSlots) throw HipError(BBMPC_E_INVALID, "bbmpc_gather_wait: slot must be 0 or 1");
    if (c.pending[slot]) {
        if (e->gather_deferred[slot]) {
            flush_deferred_gathers(e);                           // staged by bbmpc_optimize_gather, not enqueued yet
            host_block = 1;                                      // its staging buffer is host memory: the host has to see it consumed
        } else if (e->h_record_stage[slot] && !host_block && c.sync_mode == 1 && *(volatile const uint32_t*)c.done_flag[slot] < c.done_seq[slot]) {
            host_block = 1;                                      // ditto for an enqueued one that has not finished (rare: it is a control step old)
        }
        // about to block on the collective: should it sit in a hardware queue behind this handle's resident kernel, that kernel
        // has to go first (it would otherwise leave only when its linger time is over)
        if (host_block && e->resident_alive &&
            (c.sync_mode == 0 ? hipEventQuery(c.done[slot]) != hipSuccess : *(volatile const uint32_t*)c.done_flag[slot] < c.done_seq[slot]))
            e->resident_stop();
        if (c.sync_mode == 0) {
            if (host_block) {
                HIP_CHECK(hipEventSynchronize(c.done[slot]));
            } else {
                const hipError_t q = hipEventQuery(c.done[slot]);
                if (q == hipErrorNotReady) HIP_CHECK(hipStreamWaitEvent(e->stream, c.done[slot], 0));
                else HIP_CHECK(q);
            }
        } else {
            // normally long finished (it is a control step old): then the launch stream needs no dependency at all
            volatile const uint32_t* f = c.done_flag[slot];
            const uint32_t want = c.done_seq[slot];
            if (host_block) {
                // the collective needs every rank: a dead peer shows up as a timeout, not as a hang
                const auto t0 = std::chrono::steady_clock::now();
                while (*f < want) {
                    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120))
                        throw HipError(BBMPC_E_HIP, "bbmpc_gather_wait: record all-gather did not finish within 120 s");
                    std::this_thread::yield();
                }
            } else if (*f < want) {
                HIP_CHECK(hipStreamWaitValue32(e->stream, c.done_flag[slot], want, hipStreamWaitValueGte, 0xffffffffu));
            }
        }
        c.pending[slot] = false;
    }
    API_END
}

int bbmpc_comm_destroy(bbmpc_handle h) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->invalidate_step_graph();
    h->e->rc.destroy();
    API_END
}

}  // extern "C"

