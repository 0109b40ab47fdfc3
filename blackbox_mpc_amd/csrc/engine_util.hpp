// Host-side helpers shared by the engine's translation units (bbmpc.hip, bbmpc_cma.hip, bbmpc_mlp.hip, bbmpc_fused.hip).
#pragma once
#include <chrono>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

#include "engine.hpp"

namespace bbmpc {

inline void upload(DevBuf<float>& b, const std::vector<float>& v) {
    b.alloc(v.size());
    HIP_CHECK(hipMemcpy(b.p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
}

// A dynamics model's six normalisation vectors as the kernels read them: mean_s | std_s | mean_a | std_a | mean_t | std_t
inline std::vector<float> flatten_stats(const float* const* stats, int S, int U) {
    std::vector<float> st;
    const int lens[6] = {S, S, U, U, S, S};
    for (int i = 0; i < 6; ++i) {
        REQUIRE(stats[i], BBMPC_E_INVALID, "null statistics vector");
        st.insert(st.end(), stats[i], stats[i] + lens[i]);
    }
    return st;
}

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: set it once per (device, kernel)
// -- a process may hold handles on several devices (bbmpc_config.device).
inline void ensure_max_lds(const void* fn, int bytes) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    HIP_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    if (done.find({dev, fn}) == done.end()) {
        HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        done.insert({dev, fn});
    }
}

// kernels whose dynamic LDS grows with the population (an agent's rewards, Nst floats): past the 64 KB default they need
// the attribute raised
// static_bytes: what the kernel declares as static __shared__ on top (the two together must fit the CU's 160 KB)
inline void want_lds(const void* fn, size_t bytes, size_t static_bytes = 0) {
    if (bytes > 64 * 1024) {
        REQUIRE(bytes + static_bytes <= 159 * 1024, BBMPC_E_UNSUPPORTED, "population too large for one CU's LDS");
        ensure_max_lds(fn, (int)(159 * 1024 - static_bytes));
    }
}


// Launch the last kernel of a control step.  When the caller asked for a completion event (the record all-gather
// waits on it from its own stream) the event rides on the kernel's own dispatch packet: a separate
// hipEventRecord costs the launch stream ~5 us per control step (tools/gather_overhead.py).
template <class F, class... Args>
inline void launch_with_tail(Engine& e, F fn, dim3 grid, dim3 block, size_t lds, const Args&... args) {
    if (e.tail.event) {
        hipExtLaunchKernelGGL(fn, grid, block, lds, e.stream, nullptr, e.tail.event, 0, args...);
        e.tail.attached = true;
    } else {
        hipLaunchKernelGGL(fn, grid, block, lds, e.stream, args...);
    }
}

// The producer's side of Engine::tail, for the length of one optimize_dev: installs the request, and the handle is
// back to the empty hand-off when the scope ends -- by return or by exception -- so no later control step can publish
// into this call's memory.
class TailRequest {
    Engine& e_;
public:
    TailRequest(Engine& e, uint32_t* flag, uint32_t* count, uint32_t value) : e_(e) { e.tail = TailHandoff{flag, count, value, nullptr, false}; }
    TailRequest(Engine& e, hipEvent_t event) : e_(e) { e.tail = TailHandoff{nullptr, nullptr, 0, event, false}; }
    TailRequest(const TailRequest&) = delete;
    TailRequest& operator=(const TailRequest&) = delete;
    ~TailRequest() { e_.tail = TailHandoff{}; }
    bool taken() const { return e_.tail.attached; }       // the step's last kernel carries the hand-off
};

// The other per-call requests that optimize_dev's callers leave in Engine members (linger_launch, stage_state_src,
// in_flight_hook): set for the scope, back to "no request" on every way out of it.
template <class T>
class ScopedRequest {
    T& slot_;
public:
    ScopedRequest(T& slot, T v) : slot_(slot) { slot_ = v; }
    ScopedRequest(const ScopedRequest&) = delete;
    ScopedRequest& operator=(const ScopedRequest&) = delete;
    ~ScopedRequest() { slot_ = T{}; }
};

// ... and for a request that the launch itself uses up (subset_n): cleared only when the scope is left early, by an
// exception -- the ordinary way out says done().
template <class T>
class ClearOnThrow {
    T& slot_;
    bool done_ = false;
public:
    explicit ClearOnThrow(T& slot) : slot_(slot) {}
    ClearOnThrow(const ClearOnThrow&) = delete;
    ClearOnThrow& operator=(const ClearOnThrow&) = delete;
    void done() { done_ = true; }
    ~ClearOnThrow() { if (!done_) slot_ = T{}; }
};

// Spin until done() holds.  The clock is looked at every 4096 spins; after 2 s last_look() -- the caller's "settle what
// may still be running, then look once more" -- decides: it returns whether the wait is over (or throws).  Returns
// false only when last_look() said so.
template <class Done, class LastLook>
inline bool spin_until(std::chrono::steady_clock::time_point t0, Done done, LastLook last_look) {
    uint32_t spins = 0;
    while (!done()) {
        if ((++spins & 0xfff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) return last_look();
    }
    return true;
}

// every translation unit has its own copy of the truncated-normal quantile table (rng.hpp, `static __device__`): the
// core uploads all of them when a handle is created on a device for the first time
void bbmpc_tu_cma_upload_tnq(const float2* table);
void bbmpc_tu_mlp_upload_tnq(const float2* table);
void bbmpc_tu_fused_upload_tnq(const float2* table);
void note_resident_handle();          // a handle published a resident kernel's mailbox (stop_foreign_residents counts them)

}  // namespace bbmpc
