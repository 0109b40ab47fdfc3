#!/usr/bin/env python
"""Host time of one control-step call with the GPU taken out: a stub with bbmpc_optimize's signature (compiled on the fly
with the system C compiler; it only writes its outputs) stands in for the library, and the same call is timed through

  the bare ctypes foreign call with cached pointers,
  Engine.optimize's ctypes body              (BBMPC_FASTCALL=0),
  Engine.optimize through the _fastcall extension,
  MPCPolicy.act on top of each.

CPU only, no GPU is touched.  usage: host_call_overhead.py [calls]   (default 200000; A = 1, S = 3, U = 1)"""
import ctypes
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STUB = r"""
#include <stdint.h>
int bbmpc_optimize(void* h, const float* state, int32_t t, int32_t noise, float* action, float* next_state, float* reward) {
    (void)h; (void)t; (void)noise;
    action[0] = state[0]; next_state[0] = state[0]; next_state[1] = state[1]; next_state[2] = state[2]; reward[0] = state[2];
    return 0;
}
int bbmpc_optimize_gather(void* h, const float* state, int32_t t, int32_t noise, float* action, float* next_state, float* reward,
                          float* d_gathered, int32_t slot) {
    (void)d_gathered; (void)slot;
    return bbmpc_optimize(h, state, t, noise, action, next_state, reward);
}
"""


def per_call_us(f, n):
    for _ in range(min(n, 2000)):
        f()
    best = float("inf")
    for _ in range(3):                                   # the best of three passes: the machine's other work only adds
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        best = min(best, (time.perf_counter() - t0) / n)
    return best * 1e6


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 200000
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.optimizers import CEMOptimizer
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import PendulumTrueModel, pendulum_reward_function

    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if not cc:
        raise SystemExit("host_call_overhead.py: no C compiler (cc / gcc / clang) for the stub")
    d = tempfile.mkdtemp(prefix="bbmpc_stub_")
    with open(os.path.join(d, "stub.c"), "w") as f:
        f.write(STUB)
    subprocess.run([cc, "-O2", "-shared", "-fPIC", os.path.join(d, "stub.c"), "-o", os.path.join(d, "libstub.so")], check=True)
    stub = ctypes.CDLL(os.path.join(d, "libstub.so"))
    stub.bbmpc_optimize.argtypes = L.lib.bbmpc_optimize.argtypes
    stub.bbmpc_optimize_gather.argtypes = L.lib.bbmpc_optimize_gather.argtypes
    token = ctypes.c_int64(0)

    class StubEngine(Engine):                            # Engine's hot path on the stub; nothing else of it is used
        def __init__(self, fastcall):
            self._h = ctypes.c_void_p(ctypes.addressof(token))
            self._lib, self.A, self.S, self.U, self._fastcall_on = stub, 1, 3, 1, fastcall
            self.cfg = L.Config()
            self.cfg.dynamics, self.cfg.reward = L.DYN_PENDULUM, L.REW_PENDULUM

        def close(self):
            self._fast = None

    act_space, obs_space = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])

    def policy(eng):
        """MPCPolicy over the stub engine: the objects act() and OptimizerBase.__call__ walk through, no handle created."""
        handler = SystemDynamicsHandler(act_space, obs_space, true_model=True, dynamics_function=PendulumTrueModel())
        opt = CEMOptimizer(env_action_space=act_space, env_observation_space=obs_space, num_agents=1, planning_horizon=30,
                           population_size=500, max_iterations=5, num_elite=50)
        opt._trajectory_evaluator = DeterministicTrajectoryEvaluator(reward_function=pendulum_reward_function,
                                                                     system_dynamics_handler=handler)
        opt._engine = eng
        eng._dyn_version = (getattr(handler._dynamics_function, "_version", 0), handler._version)
        pol = MPCPolicy.__new__(MPCPolicy)
        pol._optimizer, pol._refine_steps, pol._act_call_counter = opt, 0, 0
        return pol

    obs = np.array([[0.5, 0.25, -1.0]], np.float32)
    rows = []
    slow, fast = StubEngine(False), StubEngine(True)
    st, action, nxt, rew, p_st, p_act, p_nxt, p_rew = slow._io_buffers()
    st[:] = obs
    fn, h = stub.bbmpc_optimize, slow._h
    rows.append(("bare ctypes call, cached pointers", per_call_us(lambda: fn(h, p_st, 0, 0, p_act, p_nxt, p_rew), n)))
    rows.append(("Engine.optimize, ctypes body (BBMPC_FASTCALL=0)", per_call_us(lambda: slow.optimize(obs, 0), n)))
    have = bool(fast._bind_fast())
    if have:
        bound = fast._fast
        rows.append(("_fastcall bound.optimize, called directly", per_call_us(lambda: bound.optimize(obs, 0, False), n)))
        rows.append(("Engine.optimize, _fastcall extension", per_call_us(lambda: fast.optimize(obs, 0), n)))
    pol_slow, pol_fast = policy(slow), policy(fast)
    rows.append(("MPCPolicy.act over the ctypes body", per_call_us(lambda: pol_slow.act(obs, 0), n)))
    if have:
        rows.append(("MPCPolicy.act over the _fastcall extension", per_call_us(lambda: pol_fast.act(obs, 0), n)))
    else:
        print("the _fastcall extension is not built: only the ctypes rows are measured")
    print("host time per call, stub library, A=1 S=3 U=1, %d calls (best of 3 passes)" % n)
    for name, us in rows:
        print("  %-52s %6.2f us" % (name, us))


if __name__ == "__main__":
    main()
