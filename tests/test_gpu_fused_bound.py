"""k_fused_pendulum's two launch bounds: the 512-thread form (256 VGPRs a wave; CEM with the samples in LDS, workgroups of
up to 512 threads) against the 1024-thread form, which BBMPC_FUSED_BOUND=1024 keeps at every size.  The 512-thread form
also runs CEM's tail in front of the last statistics barrier.  None of that may change a bit: every test runs the same
handle configuration under BBMPC_FUSED_BOUND=512 and =1024 with the same seed (and, where the entry point takes them, the
same injected draws) and compares action, next state, reward and the carried mean / variance bit for bit.

The switch is read when a handle is created.  Caller-injected draws go through the INJ = 1 instantiations (launch per
call only: a resident kernel reads prefetched draws), which have both forms as well."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0x5EEDB0D512
LO, HI = [-2.0], [2.0]
CALLS = 4


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _engine(L, monkeypatch, bound, N, H=30, iters=5, k=50, resident=True, opt="CEM", lo=LO, hi=HI):
    """the environment is read when the handle is created"""
    from blackbox_mpc_amd.engine import Engine
    monkeypatch.setenv("BBMPC_FUSED", "1")
    if resident:
        monkeypatch.delenv("BBMPC_LINGER_US", raising=False)
    else:
        monkeypatch.setenv("BBMPC_LINGER_US", "0")
    if bound is None:
        monkeypatch.delenv("BBMPC_FUSED_BOUND", raising=False)
    else:
        monkeypatch.setenv("BBMPC_FUSED_BOUND", str(bound))
    eng = Engine({"CEM": L.OPT_CEM, "PI2": L.OPT_PI2}[opt], L.DYN_PENDULUM, L.REW_PENDULUM, lo, hi, dim_s=3, num_agents=1,
                 planning_horizon=H, population_size=N, max_iterations=iters, num_elite=k if opt == "CEM" else 0, seed=SEED)
    monkeypatch.delenv("BBMPC_FUSED_BOUND", raising=False)
    return eng


START = np.array([[np.cos(2.6), np.sin(2.6), 0.4]], np.float32)


def _loop(eng, calls=CALLS, noise=False, start=START):
    """closed loop, host in / host out, nothing else called between the steps; then the carried distribution"""
    s = start
    out = []
    for t in range(calls):
        a, s, r = eng.optimize(s, t, add_exploration_noise=noise)
        out.append((a.copy(), s.copy(), r.copy()))
    return out, eng.get_state("mean"), eng.get_state("var")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _same(got, want, what):
    (g_steps, g_mean, g_var), (w_steps, w_mean, w_var) = got, want
    assert len(g_steps) == len(w_steps)
    for t, (g, w) in enumerate(zip(g_steps, w_steps)):
        for x, y, item in zip(g, w, ("action", "next state", "reward")):
            np.testing.assert_array_equal(_bits(x), _bits(y), err_msg="%s call %d %s" % (what, t, item))
    np.testing.assert_array_equal(_bits(g_mean), _bits(w_mean), err_msg=what + " get_state(mean)")
    np.testing.assert_array_equal(_bits(g_var), _bits(w_var), err_msg=what + " get_state(var)")


def _form(eng):
    """the launch bound in the instantiation's name: k_fused_pendulum<OPT, SAMPLES_LDS, FASTM, INJ, ILP, MAXT, LINGER>"""
    inst = eng.profile_instantiation()
    assert inst.startswith("k_fused_pendulum<"), inst
    return int(inst[:-1].split(",")[5])


def _pair(L, monkeypatch, what, prepare=None, forms=(512, 1024), **kw):
    """the same configuration under both settings of the switch; returns the two results' first steps for further checks"""
    loop_kw = {k: kw.pop(k) for k in ("calls", "noise", "start") if k in kw}
    res = []
    for bound, form in zip((512, 1024), forms):
        eng = _engine(L, monkeypatch, bound, **kw)
        if prepare:
            prepare(eng)
        res.append(_loop(eng, **loop_kw))
        assert _form(eng) == form, (what, bound, eng.profile_instantiation())
        resident = kw.get("resident", True) and not prepare
        assert eng.profile_instantiation().endswith("true>") == resident, (what, eng.profile_instantiation())
        eng.close()
    _same(res[0], res[1], what)
    return res[0]


# N = 500: not a multiple of 64; 512; 449: the smallest N with Nst = 512 (the compile-time sample stride); 448: Nst = 448,
# the run-time-stride body; 64: one wave
@pytest.mark.parametrize("N", [500, 512, 449, 448, 64])
def test_cem_resident(L, monkeypatch, N):
    _pair(L, monkeypatch, "resident N=%d" % N, N=N)


# H = 7: one block of four model steps plus three remainder steps, no full trip; H = 30 with one iteration: the early tail
# and the first iteration coincide
@pytest.mark.parametrize("H,iters", [(30, 5), (7, 5), (4, 5), (30, 1)])
def test_cem_launch_per_call(L, monkeypatch, H, iters):
    _pair(L, monkeypatch, "launched H=%d iters=%d" % (H, iters), N=500, H=H, iters=iters, resident=False)


# k = 64: the last size whose elites stay in a lane's registers; 65: the generic statistics loop
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
@pytest.mark.parametrize("k", [1, 64, 65, 500])
def test_num_elite(L, monkeypatch, k, resident):
    _pair(L, monkeypatch, "k=%d resident=%s" % (k, resident), N=500, k=k, resident=resident)


def test_ties_every_reward_equal(L, monkeypatch):
    """all draws zero: every candidate is the mean, min == bound, no radix pass runs (the selection's pass == 0 path)"""
    N, H, iters = 500, 30, 5
    zeros = np.zeros((iters, N, 1, H, 1), np.float32)
    _pair(L, monkeypatch, "all-zero draws", prepare=lambda e: e.inject_noise(L.NOISE_TRUNC_NORMAL, zeros), N=N, H=H, iters=iters,
          resident=False, calls=2)


def test_ties_every_reward_equal_on_prefetched_draws(L, monkeypatch):
    """the same on the resident form, which takes no injected draws: bounds of zero width leave every candidate at the mean"""
    _pair(L, monkeypatch, "zero-width bounds", N=500, lo=[0.5], hi=[0.5])


def test_ties_more_than_k_share_the_better_of_two_rewards(L, monkeypatch):
    """two distinct candidates, 250 of each, interleaved: far more than k = 50 share the better reward, so the k-th key is
    pinned with no low bit left and the exact-tie path picks the lowest indices"""
    N, H, iters = 500, 30, 5
    draws = np.zeros((iters, N, 1, H, 1), np.float32)
    draws[:, 1::2] = 1.0
    first = _pair(L, monkeypatch, "two rewards", prepare=lambda e: e.inject_noise(L.NOISE_TRUNC_NORMAL, draws), N=N, H=H, iters=iters,
                  resident=False, calls=2)
    assert np.all(np.isfinite(first[1]))


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
def test_nan_start_state(L, monkeypatch, resident):
    """every candidate's reward sum is NaN, hence -1e6 (deterministic.py:75-77): one more population of equal rewards; the
    record's next state and reward are NaN, and every call returns.

    The NaNs are compared bit for bit too: a tail whose model step the compiler had rewritten as 3u - 15 sin (for
    -15 sin + 3u) gave the next state's angular velocity as 0xffc00000 where the 1024-thread form gives 0x7fc00000."""
    start = np.array([[np.nan, 0.0, 0.0]], np.float32)
    steps, mean, _ = _pair(L, monkeypatch, "NaN start resident=%s" % resident, N=500, resident=resident, start=start)
    for a, s, r in steps:
        assert np.isfinite(a).all() and np.isnan(s).any() and np.isnan(r).all()
    assert np.isfinite(mean).all()


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "launched"])
@pytest.mark.parametrize("xi", ["drawn", "injected"])
def test_exploration_noise_on(L, monkeypatch, resident, xi):
    """the early tail applies the same exploration term"""
    prepare = None
    if xi == "injected":
        prepare = lambda e: e.inject_noise(L.NOISE_EXPLORATION, np.array([[0.7]], np.float32))      # noqa: E731
    res = []
    for bound in (512, 1024):
        eng = _engine(L, monkeypatch, bound, N=500, resident=resident)
        if prepare:
            prepare(eng)
        res.append(_loop(eng, noise=True))
        assert _form(eng) == bound and eng.profile_instantiation().endswith("true>") == resident
        eng.close()
    _same(res[0], res[1], "noise on, %s, resident=%s" % (xi, resident))
    # and the term is applied at all: the same closed loop without it differs
    eng = _engine(L, monkeypatch, 512, N=500, resident=resident)
    quiet = _loop(eng)
    eng.close()
    assert not np.array_equal(_bits(quiet[0][0][0]), _bits(res[0][0][0][0]))


@pytest.mark.parametrize("bound", [None, 512, 1024])
def test_selection_rule(L, monkeypatch, bound):
    """a workgroup of more than 512 threads, and every optimizer but CEM, runs the 1024-thread form whatever the switch says;
    N = 500 runs the 512-thread form unless the switch says 1024"""
    for kw in (dict(N=513), dict(N=1000, opt="PI2")):
        for resident in (True, False):
            eng = _engine(L, monkeypatch, bound, resident=resident, **kw)
            _loop(eng, calls=2)
            assert _form(eng) == 1024, (kw, bound, eng.profile_instantiation())
            eng.close()
    for resident in (True, False):
        eng = _engine(L, monkeypatch, bound, N=500, resident=resident)
        _loop(eng, calls=2)
        assert _form(eng) == (1024 if bound == 1024 else 512), (bound, eng.profile_instantiation())
        eng.close()


def test_switch_takes_512_and_1024_only(L, monkeypatch):
    with pytest.raises(Exception, match="BBMPC_FUSED_BOUND"):
        _engine(L, monkeypatch, 256, N=500)


def test_traced_elite_sets(L, monkeypatch):
    """with tracing on a control step is launched (no resident kernel) and the sorted elite list is produced as well"""
    N, iters, k = 500, 5, 50
    got = []
    for bound in (512, 1024):
        eng = _engine(L, monkeypatch, bound, N=N, iters=iters, k=k)
        eng.set_trace(True)
        steps = _loop(eng, calls=2)
        assert eng.call_stats()[0] == 0 and not eng.profile_instantiation().endswith("true>")
        got.append((steps, [eng.get_trace(it, L.TRACE_ELITES).copy() for it in range(iters)],
                    [eng.get_trace(it, L.TRACE_REWARDS).copy() for it in range(iters)]))
        eng.close()
    _same(got[0][0], got[1][0], "traced")
    for it in range(iters):
        np.testing.assert_array_equal(got[0][1][it], got[1][1][it], err_msg="elites of iteration %d" % it)
        np.testing.assert_array_equal(_bits(got[0][2][it]), _bits(got[1][2][it]), err_msg="rewards of iteration %d" % it)
        assert len(set(got[0][1][it].ravel().tolist())) == k
