"""Every form of the persistent pendulum kernel's prefetched-draws rollout loop (kernels_fused.hpp, INJ == 2).

The loop takes two blocks of four model steps a trip, then a single block, then up to three remainder steps; the draws of
block b + 2 and sigma / mean of block b + 1 are loaded while block b runs; the quirk-Q1 flag and the row stride of the
stored samples are decided once per launch (a compile-time stride for Nst = 512, the run-time one otherwise).  None of it
may change a bit:

 * prefetched draws against in-kernel draws (the generic loop: another code path, the same Philox counters), over every
   loop exit -- H = 1, 3 (no block), 4, 7 (one block, remainders 0 and 3), 8, 9, 12, 13, 15, 16, 17 (every residue of the
   block count modulo 4 and every remainder behind an even and an odd count), 30 (the workload) -- and populations of one
   lane, one wave minus / plus one, the workload's 500 (Nst = 512: the compile-time stride) and 1100 (above the launch's
   1024 threads: a lane rolls out a second trajectory);
 * both settings of quirk Q1 against the oracle, with the evaluator tests' tolerances and helper (tests/parity_util.py);
 * the resident pass against a launch per call, 20 closed-loop calls at N = 500, H = 30;
 * the timing-only knob BBMPC_BALANCE.
"""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests.parity_util import assert_pendulum_rewards

pytestmark = pytest.mark.gpu
F = np.float32
LO, HI = [-2.0], [2.0]
R_RTOL, R_ATOL = 2e-4, 2e-3          # H-step summed rewards: tests/test_gpu_pendulum.py


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _engine(L, opt, A, H, N, iters, k, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=iters, num_elite=k, **kw)


def _closed_loop(eng, steps, reset_at=None):
    s = O.pendulum_start_states(eng.A)
    out = []
    for t in range(steps):
        if t == reset_at:
            eng.reset()
        a, s, r = eng.optimize(s)
        out.append(np.concatenate([np.ravel(a), np.ravel(s), np.ravel(r)]))
    return np.stack(out)


HS = [1, 3, 4, 7, 8, 9, 12, 13, 15, 16, 17, 30]
CASES = [(o, H) for o in ("CEM", "PI2") for H in HS] + [("RandomSearch", 7), ("RandomSearch", 30)]


@pytest.mark.parametrize("N", [1, 63, 65, 500, 1100])
@pytest.mark.parametrize("opt_name,H", CASES)
def test_prefetched_draws_match_in_kernel_draws_at_every_loop_exit(L, monkeypatch, opt_name, H, N):
    # the comparison of test_noise_prefetch_is_bit_identical_to_in_kernel_draws (tests/test_gpu_pendulum.py): 10 control
    # steps cross a boundary of the 8-step prefetch chunks, with a reset() on the way
    opt = {"CEM": L.OPT_CEM, "PI2": L.OPT_PI2, "RandomSearch": L.OPT_RANDOM_SEARCH}[opt_name]
    monkeypatch.setenv("BBMPC_FUSED", "1")
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("BBMPC_NOISE_PREFETCH", mode)
        eng = _engine(L, opt, 1, H, N, 3, max(N // 10, 1), seed=11)
        runs[mode] = _closed_loop(eng, 10, reset_at=6)
        eng.close()
    np.testing.assert_array_equal(runs["0"], runs["1"])


@pytest.mark.parametrize("fix_q1", [False, True])
@pytest.mark.parametrize("N,H", [(500, 7), (500, 30), (200, 7), (200, 30)])
def test_both_settings_of_quirk_q1_against_the_oracle(L, monkeypatch, N, H, fix_q1):
    # the rewards the rollout loop sums (traced, with the samples it stored) against the oracle's evaluation of the same
    # samples: quirk Q1 as executed (0.001 * sum(next_state ** 2)) and as declared (0.001 * sum(action ** 2)).
    # N = 500 stores with the compile-time stride, N = 200 with the run-time one.
    monkeypatch.setenv("BBMPC_FUSED", "1")
    A, iters = 2, 2
    eng = _engine(L, L.OPT_CEM, A, H, N, iters, max(N // 10, 1), seed=5, quirks=L.FIX_Q1_REWARD_ARG_ORDER if fix_q1 else 0)
    eng.set_trace(True)
    states = O.pendulum_start_states(A)
    eng.optimize(states)
    reward = (lambda c, a, n: O.pendulum_reward(c, a, n, as_executed=False)) if fix_q1 else "pendulum"
    ev = O.Evaluator(reward, O.Handler(O.pendulum_dynamics, True))
    for it in range(iters):
        samples = eng.get_trace(it, L.TRACE_SAMPLES)
        got = eng.get_trace(it, L.TRACE_REWARDS)
        assert samples.shape == (N, A, H, 1) and got.shape == (N, A)
        assert_pendulum_rewards(got, ev(states, samples), states, samples, R_RTOL, R_ATOL, as_executed=not fix_q1,
                                what="N=%d H=%d fix_q1=%s it=%d" % (N, H, fix_q1, it))
    eng.close()


def _twenty_calls(L, monkeypatch, env):
    for k, v in env.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    eng = _engine(L, L.OPT_CEM, 1, 30, 500, 5, 50, seed=3)
    out = _closed_loop(eng, 20)
    stats = eng.call_stats()
    eng.close()
    return out, stats


@pytest.fixture(scope="module")
def launch_per_call_reference(L):
    mp = pytest.MonkeyPatch()
    try:
        out, (served, launched) = _twenty_calls(L, mp, {"BBMPC_FUSED": "1", "BBMPC_LINGER_US": "0", "BBMPC_BALANCE": None})
    finally:
        mp.undo()
    assert (served, launched) == (0, 20)
    return out


def test_resident_pass_matches_launch_per_call(L, monkeypatch, launch_per_call_reference):
    got, (served, launched) = _twenty_calls(L, monkeypatch, {"BBMPC_FUSED": "1", "BBMPC_LINGER_US": None, "BBMPC_BALANCE": None})
    print("served %d launched %d" % (served, launched))
    assert served + launched == 20 and served > 0                # the resident form did run
    np.testing.assert_array_equal(got, launch_per_call_reference)


@pytest.mark.parametrize("linger", ["resident", "launch"])
@pytest.mark.parametrize("balance", ["0", "1"])
def test_timing_only_knobs_change_no_bits(L, monkeypatch, launch_per_call_reference, balance, linger):
    got, _ = _twenty_calls(L, monkeypatch, {"BBMPC_FUSED": "1", "BBMPC_BALANCE": balance,
                                           "BBMPC_LINGER_US": None if linger == "resident" else "0"})
    np.testing.assert_array_equal(got, launch_per_call_reference)
