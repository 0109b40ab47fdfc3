// What the C ABI entry points (include/bbmpc.h) share, whichever translation unit defines them.
#pragma once
#include "engine.hpp"
#include "host_stage_layout.hpp"

namespace bbmpc {
extern thread_local std::string g_last_error;     // bbmpc_last_error (bbmpc.hip)
void stop_foreign_residents(Engine* self);
}  // namespace bbmpc

using bbmpc::Engine;
using bbmpc::HipError;

struct bbmpc_handle_s {
    Engine* e;
};

#define API_BEGIN try {
#define API_END                                   \
    }                                             \
    catch (const HipError& ex) {                  \
        bbmpc::g_last_error = ex.what();          \
        return ex.code;                           \
    }                                             \
    catch (const std::exception& ex) {            \
        bbmpc::g_last_error = ex.what();          \
        return BBMPC_E_INVALID;                   \
    }                                             \
    return BBMPC_OK;

// Every entry point runs with the handle's device current and leaves the caller's current device as it found it: a
// process may hold handles on several GPUs (bbmpc_config.device) next to a PyTorch caller with its own idea of the
// current device; lazy allocations, stream / event creation, hipFuncSetAttribute and launches all bind to "current".
struct DeviceGuard {
    int prev = -1;
    bool restore = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev && dev >= 0) {
            HIP_CHECK(hipSetDevice(dev));
            restore = true;
        }
    }
    ~DeviceGuard() {
        if (restore) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

// How a host-in / host-out entry point reaches its device-pointer twin: declare the tensors; upload()
// sizes the handle's one staging buffer (Engine::d_stage) and enqueues the copies in; st[slot] is the device pointer;
// finish() enqueues the copies out and waits once -- all on the handle's stream.  Refusals come before upload(): until
// then nothing is allocated or copied.  A stage opened inside a live one (a host callback) keeps a buffer of its own.
class HostStage {
    Engine& e_;
    bbmpc::DevBuf<float> nested_;
    bbmpc::DevBuf<float>& buf_;
    bbmpc::StageLayout lay_;
    const float* src_[bbmpc::StageLayout::kMaxSlots];
    float* dst_[bbmpc::StageLayout::kMaxSlots];
    int add(const float* src, float* dst, size_t count, bool wanted, size_t align = 1) {
        const int s = lay_.add(count, wanted, align);
        src_[s] = src; dst_[s] = dst;
        return s;
    }
public:
    explicit HostStage(Engine& e) : e_(e), buf_(e.stage_depth++ == 0 ? e.d_stage : nested_) {}
    ~HostStage() { --e_.stage_depth; }
    HostStage(const HostStage&) = delete;
    HostStage& operator=(const HostStage&) = delete;
    int in(const float* host, size_t count) { return add(host, nullptr, count, host != nullptr); }     // (NULL: an empty slot, st[slot] == nullptr)
    int out(float* host, size_t count) { return add(nullptr, host, count, host != nullptr); }
    int inout(float* host, size_t count, size_t align = 1) { return add(host, host, count, host != nullptr, align); }
    int scratch(size_t count) { return add(nullptr, nullptr, count, true); }
    void upload() {
        if (buf_.n < lay_.total) {
            HIP_CHECK(hipStreamSynchronize(e_.stream));        // nothing in flight reads the buffer that is freed
            buf_.alloc(lay_.total);
        }
        for (int s = 0; s < lay_.n; ++s)
            if (src_[s] && lay_.len[s]) HIP_CHECK(hipMemcpyAsync((*this)[s], src_[s], lay_.len[s] * 4, hipMemcpyHostToDevice, e_.stream));
    }
    float* operator[](int slot) const { return lay_.at(buf_.p, slot); }
    void finish() {
        for (int s = 0; s < lay_.n; ++s)
            if (dst_[s] && lay_.len[s]) HIP_CHECK(hipMemcpyAsync(dst_[s], (*this)[s], lay_.len[s] * 4, hipMemcpyDeviceToHost, e_.stream));
        HIP_CHECK(hipStreamSynchronize(e_.stream));
    }
};

// The download half alone (the dump_noise family): fill(device pointer) launches what writes the `count` floats.
template <class Fill>
inline void stage_read_back(Engine& e, float* out, size_t count, Fill fill) {
    HostStage st(e);
    const int d = st.out(out, count);
    st.upload();
    fill(st[d]);
    HIP_CHECK(hipGetLastError());
    st.finish();
}

#define CHECK_HANDLE_NOSETTLE(h)                                            \
    if (!(h) || !(h)->e) throw HipError(BBMPC_E_INVALID, "null handle");    \
    DeviceGuard _device_guard((h)->e->device);                              \
    bbmpc::stop_foreign_residents((h)->e)
#define CHECK_HANDLE(h)        \
    CHECK_HANDLE_NOSETTLE(h);  \
    (h)->e->settle()
#define CHECK_PTR(p) \
    if (!(p)) throw HipError(BBMPC_E_INVALID, "null pointer argument: " #p)
