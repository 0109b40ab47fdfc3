"""The resident pendulum kernel publishes first and keeps its books afterwards: the record travels in a self-validating
completion line, the exploration term is staged ahead of the tail, CEM's wave 0 runs the tail in front of its last barrier,
and mean / var / prev_mean are stored behind the publish.  None of that may change a bit: the same handle configuration is
run resident (default linger time) and launched per call (BBMPC_LINGER_US=0), closed loop, and every action, next state,
reward and, at the end, the carried optimizer state is compared bit for bit.

Shapes are tiny on purpose: N = 70 (a ragged last wave), H = 6 (one full block of four model steps plus two remainder
steps), 2 iterations, k = 8."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N, H, ITERS, K = 70, 6, 2, 8
SEED = 0x0C0FFEE123456789
CALLS = 12
LO, HI = [-2.0], [1.5]


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _opt(L, name):
    return {"CEM": (L.OPT_CEM, 0), "CEM-warm": (L.OPT_CEM, L.FIX_Q2_CEM_WARM_START), "PI2": (L.OPT_PI2, 0),
            "RS": (L.OPT_RANDOM_SEARCH, 0), "SPSA": (L.OPT_SPSA, 0)}[name]


def _engine(L, monkeypatch, name, A, resident, iters=ITERS, env=None):
    """the environment is read when the handle is created"""
    from blackbox_mpc_amd.engine import Engine
    monkeypatch.setenv("BBMPC_FUSED", "1")
    if resident:
        monkeypatch.delenv("BBMPC_LINGER_US", raising=False)
    else:
        monkeypatch.setenv("BBMPC_LINGER_US", "0")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    opt, quirks = _opt(L, name)
    eng = Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H, population_size=N,
                 max_iterations=iters, num_elite=K, seed=SEED, quirks=quirks)
    for k in (env or {}):
        monkeypatch.delenv(k)
    return eng


def _start(A):
    th = np.linspace(0.3, 2.9, A, dtype=np.float32)
    return np.stack([np.cos(th), np.sin(th), np.linspace(-1.0, 1.0, A, dtype=np.float32) if A > 1 else np.zeros(1, np.float32)], 1).astype(np.float32)


def _xi(A):
    return np.linspace(-1.7, 1.9, A, dtype=np.float32).reshape(A, 1)


def _loop(L, eng, A, noise, calls=CALLS):
    """closed loop, host in / host out, nothing else called between the steps"""
    if noise == "injected":
        eng.inject_noise(L.NOISE_EXPLORATION, _xi(A))
    s = _start(A)
    out = []
    for t in range(calls):
        a, s, r = eng.optimize(s, t, add_exploration_noise=noise != "off")
        out.append((a.copy(), s.copy(), r.copy()))
    return out


def _same(got, want, what):
    assert len(got) == len(want)
    for t, (g, w) in enumerate(zip(got, want)):
        for x, y, item in zip(g, w, ("action", "next state", "reward")):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg="%s call %d %s" % (what, t, item))


def _same_state(L, res, per, name, what):
    names = ["mean", "var"] if name != "RS" else []
    if name in ("CEM-warm", "PI2", "SPSA"):
        names.append("prev_mean")
    for n in names:
        np.testing.assert_array_equal(res.get_state(n).view(np.uint32), per.get_state(n).view(np.uint32), err_msg="%s get_state(%s)" % (what, n))


@pytest.mark.parametrize("A", [1, 3])
@pytest.mark.parametrize("noise", ["off", "on", "injected"])
@pytest.mark.parametrize("name", ["CEM", "CEM-warm", "PI2", "RS", "SPSA"])
def test_resident_equals_launch_per_call(L, monkeypatch, name, noise, A):
    res = _engine(L, monkeypatch, name, A, True)
    per = _engine(L, monkeypatch, name, A, False)
    what = "%s noise=%s A=%d" % (name, noise, A)
    got = _loop(L, res, A, noise)
    want = _loop(L, per, A, noise)
    _same(got, want, what)
    served, launched = res.call_stats()
    assert served >= 10 and served + launched == CALLS, (served, launched)
    assert res.profile_instantiation().endswith("true>"), res.profile_instantiation()
    assert per.call_stats() == (0, CALLS)
    _same_state(L, res, per, name, what)           # stored behind the publish: settled reads must still see the last step's
    # ... and the handle goes on from that state through a launch as the launched one does
    _same(_loop(L, res, A, noise, 2), _loop(L, per, A, noise, 2), what + " after get_state")
    res.close()
    per.close()


@pytest.mark.parametrize("name", ["CEM", "PI2"])
def test_a_leaving_workgroup_leaves_a_complete_line(L, monkeypatch, name):
    # agent 1's workgroup leaves after every control step: the line of the step it served must be whole, and the subset
    # launch that follows serves exactly that agent
    A = 3
    res = _engine(L, monkeypatch, name, A, True, env={"BBMPC_LINGER_TEST_QUIT": "2"})
    per = _engine(L, monkeypatch, name, A, False)
    _same(_loop(L, res, A, "on"), _loop(L, per, A, "on"), name + " test-quit")
    served, launched = res.call_stats()
    assert served + launched == CALLS and launched >= 2, (served, launched)
    _same_state(L, res, per, name, name + " test-quit")
    res.close()
    per.close()


@pytest.mark.parametrize("noise", ["off", "on", "injected"])
@pytest.mark.parametrize("name", ["CEM", "PI2", "RS"])
def test_no_iterations_the_pass_is_only_the_tail(L, monkeypatch, name, noise):
    A = 3
    res = _engine(L, monkeypatch, name, A, True, iters=0)
    per = _engine(L, monkeypatch, name, A, False, iters=0)
    got, want = _loop(L, res, A, noise), _loop(L, per, A, noise)
    _same(got, want, "%s iters=0 noise=%s" % (name, noise))
    if noise == "off" and name != "RS":          # the untouched mean[:, 0]: the bounds' midpoint
        np.testing.assert_array_equal(got[0][0], np.full((A, 1), (LO[0] + HI[0]) / 2.0, np.float32))
    served, launched = res.call_stats()
    # RandomSearch draws its one population whatever the iteration count, so its handle keeps the prefetched draws the
    # resident form is built on; CEM / PI2 without iterations draw nothing and are launched per call on both handles
    assert (served >= 10) if name == "RS" else (served == 0), (served, launched)
    res.close()
    per.close()


@pytest.mark.parametrize("A", [1, 3])
def test_sequence_numbers_across_the_tags_wrap(L, monkeypatch, A):
    # the words of a line carry the low 16 bits of the call's sequence number: calls 0xfffa .. 0x10005
    res = _engine(L, monkeypatch, "CEM", A, True, env={"BBMPC_TEST_HOST_SEQ": str(0xfff9)})
    per = _engine(L, monkeypatch, "CEM", A, False)
    _same(_loop(L, res, A, "on"), _loop(L, per, A, "on"), "tag wrap A=%d" % A)
    served, launched = res.call_stats()
    assert served >= 10, (served, launched)
    res.close()
    per.close()
