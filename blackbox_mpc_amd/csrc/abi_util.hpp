// What the C ABI entry points (include/bbmpc.h) share, whichever translation unit defines them (bbmpc.hip, bbmpc_user.hip).
#pragma once
#include "engine.hpp"

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

#define CHECK_HANDLE_NOSETTLE(h)                                            \
    if (!(h) || !(h)->e) throw HipError(BBMPC_E_INVALID, "null handle");    \
    DeviceGuard _device_guard((h)->e->device);                              \
    bbmpc::stop_foreign_residents((h)->e)
#define CHECK_HANDLE(h)        \
    CHECK_HANDLE_NOSETTLE(h);  \
    (h)->e->settle()
#define CHECK_PTR(p) \
    if (!(p)) throw HipError(BBMPC_E_INVALID, "null pointer argument: " #p)
