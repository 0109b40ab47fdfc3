"""A stand-in for the two host-in / host-out ABI entry points, compiled on the fly with the system C compiler, and an
Engine that calls it: the marshalling of Engine.optimize / optimize_gather (ctypes body and _fastcall extension) runs
without a GPU.  The "handle" is a small struct the test owns."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np

from blackbox_mpc_amd import _lib as L
from blackbox_mpc_amd.engine import Engine

STUB_SOURCE = r"""
#include <stdint.h>
#include <time.h>
typedef struct { int32_t A, S, U, code, sleep_us; int64_t calls; uint64_t last_gathered; int32_t last_slot; } stub_handle;

static void fill(stub_handle* h, const float* state, int32_t t, int32_t noise, float* action, float* next_state, float* reward,
                 float extra) {
    for (int a = 0; a < h->A; ++a) {
        float sum = 0.0f;
        for (int s = 0; s < h->S; ++s) {
            next_state[a * h->S + s] = state[a * h->S + s] * 0.5f + (float)s + extra;
            sum += state[a * h->S + s];
        }
        for (int u = 0; u < h->U; ++u) action[a * h->U + u] = state[a * h->S + (u % h->S)] * 2.0f + (float)t + 0.25f * (float)noise + (float)u;
        reward[a] = sum + (float)(100 * a) + (float)t;
    }
}

static int leave(stub_handle* h) {
    h->calls++;
    if (h->sleep_us > 0) {
        struct timespec ts = {h->sleep_us / 1000000, (long)(h->sleep_us % 1000000) * 1000L};
        nanosleep(&ts, 0);
    }
    return h->code;
}

int bbmpc_optimize(void* hv, const float* state, int32_t t, int32_t noise, float* action, float* next_state, float* reward) {
    stub_handle* h = (stub_handle*)hv;
    if (!h) return -1;
    fill(h, state, t, noise, action, next_state, reward, 0.0f);
    return leave(h);
}

int bbmpc_optimize_gather(void* hv, const float* state, int32_t t, int32_t noise, float* action, float* next_state, float* reward,
                          float* d_gathered, int32_t slot) {
    stub_handle* h = (stub_handle*)hv;
    if (!h) return -1;
    fill(h, state, t, noise, action, next_state, reward, 1000.0f * (float)(slot + 1));
    h->last_gathered = (uint64_t)(uintptr_t)d_gathered;
    h->last_slot = slot;
    return leave(h);
}
"""


class StubHandle(ctypes.Structure):
    _fields_ = [("A", ctypes.c_int32), ("S", ctypes.c_int32), ("U", ctypes.c_int32), ("code", ctypes.c_int32),
                ("sleep_us", ctypes.c_int32), ("calls", ctypes.c_int64), ("last_gathered", ctypes.c_uint64),
                ("last_slot", ctypes.c_int32)]


_stub = []


def stub_library():
    """The stub as a ctypes library with the real entry points' argument types (built once per process)."""
    if not _stub:
        cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
        assert cc, "a C compiler is needed for the stub"
        d = tempfile.mkdtemp(prefix="bbmpc_stub_")
        src, so = os.path.join(d, "stub.c"), os.path.join(d, "libstub.so")
        with open(src, "w") as f:
            f.write(STUB_SOURCE)
        subprocess.run([cc, "-O2", "-shared", "-fPIC", src, "-o", so], check=True)
        lib = ctypes.CDLL(so)
        lib.bbmpc_optimize.argtypes = L.lib.bbmpc_optimize.argtypes
        lib.bbmpc_optimize_gather.argtypes = L.lib.bbmpc_optimize_gather.argtypes
        _stub.append(lib)
    return _stub[0]


class StubEngine(Engine):
    """Engine whose handle is a StubHandle and whose hot path calls the stub: everything else of Engine is out of reach."""

    def __init__(self, A, S, U, fastcall=True, code=0, sleep_us=0):
        self.handle = StubHandle(A, S, U, code, sleep_us, 0, 0, -1)
        self._h = ctypes.c_void_p(ctypes.addressof(self.handle))
        self._lib = stub_library()
        self.A, self.S, self.U = A, S, U
        self._fastcall_on = bool(fastcall) and os.environ.get("BBMPC_FASTCALL", "1") != "0"
        self.cfg = L.Config()
        self.cfg.reward, self.cfg.dynamics = L.REW_PENDULUM, L.DYN_PENDULUM

    def close(self):                      # (nothing of the real library to destroy)
        self._fast = None


def observation(A, S, dtype=np.float32, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (A, S)).astype(dtype)
