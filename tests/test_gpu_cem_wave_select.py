"""The all-wave route of the 512-thread CEM control step's elite selection (csrc/topk.hpp, block_topk_wave_select: every
wave scans the first histogram and tests the key it holds, no barrier behind the scan) against the route it replaces in the common
case.  BBMPC_CEM_WAVE_SELECT=0, read when a handle is created, makes the same kernel take the old route, so one library is
compared with itself: two handles with the same seed, 12 closed-loop control steps each, and action, next observation,
reward and the carried mean / variance must agree bit for bit.

Shapes (H = 30): (N, k) from one wave and k = 1 up to 512 and k = 64; (500, 65) and (513, 50) are outside the route's
conditions (k > 64; more than 512 threads: the 1024-thread form) and must agree all the same; H = 3 pads the rows to four.
Designed inputs: a NaN start state (every reward -1e6: min == bound, no pass), injected draws that repeat every trajectory
four times (exact ties across the k-th key: the route must decline), launch per call as well as resident.
With the sorted elites traced the old route runs: the traces are the same under either setting.
Which route ran: bit 8 of BBMPC_TRACE_TOPK_PASSES, visible under the test hook BBMPC_TRACE_SELECT_ONLY=1.  Over 64 control
steps of the benchmark's configuration the selections that took the new route are exactly those for which the serial loop
of tests/topk_digits_check.cpp reports one pass with the whole boundary bucket in, on the same handle's traced rewards."""
import struct
import subprocess

import numpy as np
import pytest

from tests.test_topk_digits_cpu import compile_check

pytestmark = pytest.mark.gpu
SEED = 0x5EEDCE3A
LO, HI = [-2.0], [2.0]
CALLS = 12
START = np.array([[np.cos(2.6), np.sin(2.6), 0.4]], np.float32)


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _engine(L, monkeypatch, wave, N, H=30, iters=5, k=50, resident=True, select_only=False):
    """the environment is read when the handle is created"""
    from blackbox_mpc_amd.engine import Engine
    monkeypatch.setenv("BBMPC_FUSED", "1")
    monkeypatch.delenv("BBMPC_FUSED_BOUND", raising=False)
    if resident:
        monkeypatch.delenv("BBMPC_LINGER_US", raising=False)
    else:
        monkeypatch.setenv("BBMPC_LINGER_US", "0")
    monkeypatch.setenv("BBMPC_CEM_WAVE_SELECT", "1" if wave else "0")
    if select_only:
        monkeypatch.setenv("BBMPC_TRACE_SELECT_ONLY", "1")
    else:
        monkeypatch.delenv("BBMPC_TRACE_SELECT_ONLY", raising=False)
    eng = Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=1, planning_horizon=H,
                 population_size=N, max_iterations=iters, num_elite=k, seed=SEED)
    monkeypatch.delenv("BBMPC_CEM_WAVE_SELECT", raising=False)
    monkeypatch.delenv("BBMPC_TRACE_SELECT_ONLY", raising=False)
    return eng


def _loop(eng, calls=CALLS, start=START):
    s = start
    out = []
    for t in range(calls):
        a, s, r = eng.optimize(s, t, add_exploration_noise=False)
        out.append((a.copy(), s.copy(), r.copy()))
    return out, eng.get_state("mean"), eng.get_state("var")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same(got, want, what):
    (g_steps, g_mean, g_var), (w_steps, w_mean, w_var) = got, want
    assert len(g_steps) == len(w_steps)
    for t, (g, w) in enumerate(zip(g_steps, w_steps)):
        for x, y, item in zip(g, w, ("action", "next observation", "reward")):
            np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="%s call %d %s" % (what, t, item))
    np.testing.assert_array_equal(_bits(g_mean), _bits(w_mean), err_msg=what + " get_state(mean)")
    np.testing.assert_array_equal(_bits(g_var), _bits(w_var), err_msg=what + " get_state(var)")


def _form(eng):
    inst = eng.profile_instantiation()
    assert inst.startswith("k_fused_pendulum<"), inst
    return int(inst[:-1].split(",")[5])


def _pair(L, monkeypatch, what, form=512, prepare=None, **kw):
    loop_kw = {k: kw.pop(k) for k in ("calls", "start") if k in kw}
    res = []
    for wave in (True, False):
        eng = _engine(L, monkeypatch, wave, **kw)
        if prepare:
            prepare(eng)
        res.append(_loop(eng, **loop_kw))
        assert _form(eng) == form, (what, eng.profile_instantiation())
        assert eng.profile_instantiation().endswith("true>") == (kw.get("resident", True) and not prepare), (what, eng.profile_instantiation())
        eng.close()
    _same(res[0], res[1], what)
    return res[0]


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
@pytest.mark.parametrize("N,k", [(64, 1), (65, 2), (128, 16), (449, 17), (500, 50), (512, 64)])
def test_shapes_on_the_route(L, monkeypatch, N, k, resident):
    steps, _, _ = _pair(L, monkeypatch, "N=%d k=%d resident=%s" % (N, k, resident), N=N, k=k, resident=resident)
    assert all(np.isfinite(a).all() for a, _, _ in steps)


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
def test_more_than_64_elites_keeps_the_old_route(L, monkeypatch, resident):
    _pair(L, monkeypatch, "N=500 k=65 resident=%s" % resident, N=500, k=65, resident=resident)


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
def test_more_than_512_threads_keeps_the_1024_form(L, monkeypatch, resident):
    _pair(L, monkeypatch, "N=513 k=50 resident=%s" % resident, form=1024, N=513, k=50, resident=resident)


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
def test_rows_padded_to_four(L, monkeypatch, resident):
    _pair(L, monkeypatch, "H=3 resident=%s" % resident, N=500, k=50, H=3, resident=resident)


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
def test_nan_start_state(L, monkeypatch, resident):
    """every reward is -1e6: min == bound, no radix pass, the exact tie path (the lowest indices win)"""
    start = np.array([[np.nan, 0.0, 0.0]], np.float32)
    steps, mean, _ = _pair(L, monkeypatch, "NaN start resident=%s" % resident, N=500, resident=resident, start=start)
    for a, s, r in steps:
        assert np.isfinite(a).all() and np.isnan(s).any() and np.isnan(r).all()
    assert np.isfinite(mean).all()


def _repeated_draws(L, N, H, iters):
    """every trajectory four times: the rewards come in groups of four equal values, and k = 50 is no multiple of four"""
    from oracle import oracle_np as O
    rng = np.random.default_rng(77)
    base = np.stack([O.truncated_normal_noise(rng, (N // 4, 1, H, 1)) for _ in range(iters)]).astype(np.float32)
    return np.ascontiguousarray(np.repeat(base, 4, axis=1))


def test_duplicated_trajectories_across_the_boundary(L, monkeypatch):
    """the boundary group of four holds more keys than are wanted: the route declines and the tie rule decides"""
    N, H, iters, k = 500, 30, 5, 50
    draws = _repeated_draws(L, N, H, iters)
    _pair(L, monkeypatch, "ties at the k-th key", prepare=lambda e: e.inject_noise(L.NOISE_TRUNC_NORMAL, draws), N=N, H=H, iters=iters,
          k=k, resident=False, calls=2)
    # the route did decline (and the tie is there): the route bit under the selection-only trace
    eng = _engine(L, monkeypatch, True, N=N, H=H, iters=iters, k=k, select_only=True)
    eng.set_trace(True)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, draws)
    eng.optimize(START, 0, add_exploration_noise=False)
    words = np.array([int(eng.get_trace(it, L.TRACE_TOPK_PASSES)[0]) for it in range(iters)])
    rw = eng.get_trace(0, L.TRACE_REWARDS)[:, 0]
    eng.close()
    print("route words", words)
    assert not (words & 0x100).any()
    kth = np.sort(rw)[::-1][k - 1]
    assert (rw == kth).sum() >= 4 and (rw >= kth).sum() > k


def test_traced_runs_take_the_old_route(L, monkeypatch):
    """tracing the sorted elites: the same traces under either setting, and no route bit"""
    N, iters, k = 500, 5, 50
    got = []
    for wave in (True, False):
        eng = _engine(L, monkeypatch, wave, N=N, iters=iters, k=k)
        eng.set_trace(True)
        steps = _loop(eng, calls=2)
        got.append((steps, [eng.get_trace(it, L.TRACE_ELITES).copy() for it in range(iters)],
                    [eng.get_trace(it, L.TRACE_TOPK_PASSES).copy() for it in range(iters)],
                    [eng.get_trace(it, L.TRACE_REWARDS).copy() for it in range(iters)]))
        eng.close()
    _same(got[0][0], got[1][0], "traced")
    for it in range(iters):
        np.testing.assert_array_equal(got[0][1][it], got[1][1][it], err_msg="elites of iteration %d" % it)
        np.testing.assert_array_equal(got[0][2][it], got[1][2][it], err_msg="passes of iteration %d" % it)
        np.testing.assert_array_equal(_bits(got[0][3][it]), _bits(got[1][3][it]), err_msg="rewards of iteration %d" % it)
        assert len(set(got[0][1][it].ravel().tolist())) == k
        assert int(got[0][2][it][0]) < 0x100


def test_route_share_over_64_control_steps(L, monkeypatch, tmp_path):
    """config 2 (N = 500, H = 30, 5 iterations, k = 50): the selections that took the new route are exactly those the serial
    loop reports as one pass with no key too many in the boundary bucket, on this handle's own traced rewards"""
    N, H, iters, k, steps = 500, 30, 5, 50, 64
    eng = _engine(L, monkeypatch, True, N=N, H=H, iters=iters, k=k, select_only=True)
    eng.set_trace(True)
    s = START
    words, pops = [], []
    for t in range(steps):
        _, s, _ = eng.optimize(s, t, add_exploration_noise=False)
        for it in range(iters):
            words.append(int(eng.get_trace(it, L.TRACE_TOPK_PASSES)[0]))
            pops.append(eng.get_trace(it, L.TRACE_REWARDS)[:, 0].copy())
    assert _form(eng) == 512
    eng.close()
    words = np.array(words)
    exe = compile_check(tmp_path)
    path = str(tmp_path / "rewards.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<4i", len(pops), N, k, 512))
        f.write(np.ascontiguousarray(np.stack(pops), np.float32).tobytes())
    res = subprocess.run([exe, "--passes", path], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    serial = np.array([[int(x) for x in line.split()[:2]] for line in res.stdout.splitlines()])
    want = (serial[:, 0] == 1) & (serial[:, 1] == 0)
    took = (words & 0x100) != 0
    print("new route: %d of %d selections (%.1f %%); serial loop, one pass with the whole bucket in: %d (%.1f %%)"
          % (took.sum(), took.size, 100.0 * took.mean(), want.sum(), 100.0 * want.mean()))
    np.testing.assert_array_equal(words & 0xff, serial[:, 0])
    np.testing.assert_array_equal(took, want)
    assert took.mean() == want.mean() and took.any() and not took.all()
