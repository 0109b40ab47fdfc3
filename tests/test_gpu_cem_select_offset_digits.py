"""The elite selection on offset keys with a 1024-bin first pass (csrc/topk.hpp, csrc/topk_digits.hpp), on the device.

The pattern of tests/test_gpu_cem_select_handoff.py on injected draws (N in {64, 65, 500}, H = 6, 3 iterations,
k in {1, 50, 64}, two agents):
  * the traced elites are tf.nn.top_k's (oracle_np.topk_desc) of the device's own traced rewards;
  * mean / variance / action are the same bits traced or not, persistent kernel or per-iteration kernels;
  * the traced number of radix passes (TRACE_TOPK_PASSES) of every iteration and agent equals what the serial loop of
    tests/topk_digits_check.cpp (the same header, compiled for the CPU, --passes mode) gives for the traced rewards.  The
    key range depends on how the population lies over the workgroup's threads, so the program is told the thread count:
    the persistent kernel runs ceil64(max(N, k)) threads, the per-iteration refit 256 (N <= 256) or 512 (N <= 512) --
    restated here from Engine::optimize_fused / optimize_cem.
-1e6 mixed with ordinary rewards (a key span near 2^31, 32 undecided bits in front of the first pass): a NaN start state
for one of two agents makes that agent's whole population -1e6 (per agent, not mixed); NaN DRAWS for every third particle
of the other agent's first iteration make those particles' rewards -1e6 among ordinary ones (the engine takes injected
draws as they come; a NaN action reaches the reward sum and the -1e6 rule)."""
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle_np as O
from tests.test_topk_digits_cpu import compile_check

pytestmark = pytest.mark.gpu
F = np.float32
LO, HI = [-2.0], [2.0]


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    d = tmp_path_factory.mktemp("topk_digits")
    exe = compile_check(d)

    def passes(rewards, k, nthr):
        """rewards [M, N] -> the serial loop's pass count per population"""
        rewards = np.ascontiguousarray(rewards, F)
        path = str(d / "rewards.bin")
        with open(path, "wb") as f:
            f.write(struct.pack("<4i", rewards.shape[0], rewards.shape[1], k, nthr))
            f.write(rewards.tobytes())
        res = subprocess.run([exe, "--passes", path], capture_output=True, text=True)
        assert res.returncode == 0, res.stdout + res.stderr
        return np.array([int(line.split()[0]) for line in res.stdout.splitlines()], np.int32)
    return passes


def _threads(fused, N, k):
    if fused:
        return min(1024, max(-(-max(N, k) // 64) * 64, 64))
    return 1024 if N > 512 else (512 if N > 256 else 256)


def _run(L, monkeypatch, fused, trace, noise, states, N, H, iters, k):
    monkeypatch.setenv("BBMPC_FUSED", "1" if fused else "0")
    A = states.shape[0]
    from blackbox_mpc_amd.engine import Engine
    eng = Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H,
                 population_size=N, max_iterations=iters, num_elite=k, alpha=0.25)
    eng.set_trace(trace)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, noise)
    act, nxt, rew = eng.optimize(states)
    mean, var = eng.get_state("mean"), eng.get_state("var")
    el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(iters)] if trace else None
    rw = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)] if trace else None
    ps = [eng.get_trace(it, L.TRACE_TOPK_PASSES) for it in range(iters)] if trace else None
    eng.close()
    return act, nxt, rew, mean, var, el, rw, ps


def _check_all_paths(L, monkeypatch, serial, noise, states, N, H, iters, k):
    A = states.shape[0]
    ref = _run(L, monkeypatch, True, True, noise, states, N, H, iters, k)
    for it in range(iters):
        for a in range(A):
            np.testing.assert_array_equal(ref[5][it][a], O.topk_desc(ref[6][it][:, a], k))

    def check_passes(run, fused):
        pops = np.stack([run[6][it][:, a] for it in range(iters) for a in range(A)])
        want = serial(pops, k, _threads(fused, N, k)).reshape(iters, A)
        got = np.stack(run[7])
        print("passes (%s) device %s serial %s" % ("persistent" if fused else "per-iteration", got.ravel(), want.ravel()))
        np.testing.assert_array_equal(got, want)
    check_passes(ref, True)
    for fused, trace in [(True, False), (False, False), (False, True)]:
        got = _run(L, monkeypatch, fused, trace, noise, states, N, H, iters, k)
        for x, y in zip(ref[:5], got[:5]):
            np.testing.assert_array_equal(x, y)
        if trace:
            for it in range(iters):
                np.testing.assert_array_equal(got[5][it], ref[5][it])
                np.testing.assert_array_equal(got[6][it], ref[6][it])
            check_passes(got, fused)
    return ref


def _noise(N, A, H, iters, seed):
    rng = np.random.default_rng(seed)
    return np.stack([O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]).astype(F)


@pytest.mark.parametrize("N", [64, 65, 500])
@pytest.mark.parametrize("k", [1, 50, 64])
def test_random_populations(L, monkeypatch, serial, N, k):
    H, iters, A = 6, 3, 2
    _check_all_paths(L, monkeypatch, serial, _noise(N, A, H, iters, 300 * N + k), O.pendulum_start_states(A), N, H, iters, k)


@pytest.mark.parametrize("N,k", [(65, 1), (500, 50), (500, 64)])
def test_minus_1e6_per_agent(L, monkeypatch, serial, N, k):
    """agent 1 starts from a NaN state: all of its rewards are -1e6 (span 0, no pass), agent 0's are ordinary"""
    H, iters, A = 6, 2, 2
    states = O.pendulum_start_states(A)
    states[1, 0] = np.nan
    ref = _check_all_paths(L, monkeypatch, serial, _noise(N, A, H, iters, 17 * N + k), states, N, H, iters, k)
    assert np.all(ref[6][0][:, 1] == F(-1e6)) and np.all(ref[6][0][:, 0] > F(-1e6))
    assert np.all(np.stack(ref[7])[:, 1] == 0)
    np.testing.assert_array_equal(ref[5][0][1], np.arange(k))


@pytest.mark.parametrize("N,k", [(65, 1), (500, 50), (500, 64)])
def test_minus_1e6_mixed_with_ordinary_rewards(L, monkeypatch, serial, N, k):
    """NaN draws for every third particle of agent 0 in iteration 0: -1e6 among ordinary rewards in one population"""
    H, iters, A = 6, 2, 2
    noise = _noise(N, A, H, iters, 29 * N + k)
    noise[0, 1::3, 0] = np.nan
    ref = _check_all_paths(L, monkeypatch, serial, noise, O.pendulum_start_states(A), N, H, iters, k)
    rw = ref[6][0][:, 0]
    assert np.all(rw[1::3] == F(-1e6)) and np.all(np.delete(rw, np.s_[1::3]) > F(-1e6))
    assert not set(int(e) for e in ref[5][0][0]) & set(range(1, N, 3))
