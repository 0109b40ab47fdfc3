"""The elite selection's tie rule as regression cases (topk.hpp, unchanged: no new selection path is covered here) and the
resident kernel's pre-staged hand-off between control steps (kernels_fused.hpp).

Selection.  Rewards cannot be handed to the pendulum kernels directly, so ties are built from the draws: particles that
receive the same injected draws get the same reward, bit for bit.  A first run ranks a random population; the particle at
rank k - r then lends its draws to g - 1 of the worst particles (wherever their indices fall), so that g keys tie across
the k-th place and exactly r of them are wanted (g = 1, r, r + 1, 64, 65: group sizes, not radix bucket sizes).  The traced
elites must be tf.nn.top_k's (oracle_np.topk_desc: larger first, ties to the lower index) of the device's own rewards, and
mean / variance must be the same bits traced or not, persistent kernel or per-iteration kernels.  A reward of exactly -0.0
cannot be produced this way (a sum of negative terms); -1e6 is (NaN state).

Hand-off.  20 consecutive calls of a resident handle (N = 64, H = 8; the noise chunks hold 8 control steps) against a handle
created with BBMPC_LINGER_US=0.  At a chunk's last step the kernel predicts nothing and fetches its first draws behind the
request; everywhere else the prediction holds.  A predicted pointer that is WRONG cannot be produced through the host's
entry points (control steps only advance, and a call with injected draws is a launch of the non-resident form), so of the
reload branch only the nothing-predicted case runs here; the injected variant covers the relaunches around such calls."""
import numpy as np
import pytest

from oracle import oracle_np as O

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


def _engine(L, N, H, iters, k, A=1, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, LO, HI, dim_s=3, num_agents=A, planning_horizon=H,
                  population_size=N, max_iterations=iters, num_elite=k, alpha=0.25, **kw)


def _run(L, monkeypatch, fused, trace, noise, states, N, H, iters, k):
    """One control step on injected draws -> (action, next state, reward, mean, var, traced elites or None, traced rewards or None)"""
    monkeypatch.setenv("BBMPC_FUSED", "1" if fused else "0")
    A = states.shape[0]
    eng = _engine(L, N, H, iters, k, A=A)
    eng.set_trace(trace)
    eng.inject_noise(L.NOISE_TRUNC_NORMAL, noise)
    act, nxt, rew = eng.optimize(states)
    mean, var = eng.get_state("mean"), eng.get_state("var")
    el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(iters)] if trace else None
    rw = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(iters)] if trace else None
    eng.close()
    return act, nxt, rew, mean, var, el, rw


def _check_all_paths(L, monkeypatch, noise, states, N, H, iters, k):
    ref = _run(L, monkeypatch, True, True, noise, states, N, H, iters, k)
    for it in range(iters):
        for a in range(states.shape[0]):
            np.testing.assert_array_equal(ref[5][it][a], O.topk_desc(ref[6][it][:, a], k))
    for fused, trace in [(True, False), (False, False), (False, True)]:
        got = _run(L, monkeypatch, fused, trace, noise, states, N, H, iters, k)
        for x, y in zip(ref[:5], got[:5]):
            np.testing.assert_array_equal(x, y)
        if trace:
            for it in range(iters):
                np.testing.assert_array_equal(got[5][it], ref[5][it])      # the elite set, in tf.nn.top_k's order
                np.testing.assert_array_equal(got[6][it], ref[6][it])
    return ref


def _noise(N, A, H, iters, seed):
    rng = np.random.default_rng(seed)
    return np.stack([O.truncated_normal_noise(rng, (N, A, H, 1)) for _ in range(iters)]).astype(F)


@pytest.mark.parametrize("N", [64, 65, 500])
@pytest.mark.parametrize("k", [1, 50, 64])
def test_random_populations(L, monkeypatch, N, k):
    H, iters, A = 6, 3, 2
    states = O.pendulum_start_states(A)
    _check_all_paths(L, monkeypatch, _noise(N, A, H, iters, 100 * N + k), states, N, H, iters, k)


def _tie_group(L, monkeypatch, N, k, r, g, seed):
    """g particles tied across the k-th place of iteration 0, r of them wanted; returns the draws"""
    H, iters = 6, 2
    states = O.pendulum_start_states(1)
    noise = _noise(N, 1, H, iters, seed)
    base = _run(L, monkeypatch, True, True, noise, states, N, H, iters, k)
    order = O.topk_desc(base[6][0][:, 0], N)            # all particles, best first
    lender = int(order[k - r])
    worst = [int(n) for n in order[::-1] if n != lender][:g - 1]
    assert len(worst) == g - 1 and (g == 1 or N - (g - 1) >= k)
    for n in worst:
        noise[0, n, 0] = noise[0, lender, 0]
    return noise, states, H, iters, lender, worst


@pytest.mark.parametrize("g_of_r", ["1", "r", "r+1", "64", "65"])
@pytest.mark.parametrize("N,k,r", [(500, 50, 3), (500, 64, 1), (200, 50, 7)])
def test_tie_group_across_the_kth_place(L, monkeypatch, N, k, r, g_of_r):
    g = {"1": 1, "r": r, "r+1": r + 1, "64": 64, "65": 65}[g_of_r]
    noise, states, H, iters, lender, worst = _tie_group(L, monkeypatch, N, k, r, g, seed=N + 7 * k + g)
    ref = _check_all_paths(L, monkeypatch, noise, states, N, H, iters, k)
    rw = ref[6][0][:, 0]
    group = [lender] + worst
    assert np.all(rw[group] == rw[lender])               # the same draws: the same reward, bit for bit
    want_in = sorted(group)[:min(r, g)]                  # ties go to the lower index
    el = set(int(e) for e in ref[5][0][0])
    assert all(n in el for n in want_in) and len(el & set(group)) == min(r, g)


@pytest.mark.parametrize("N,k", [(64, 1), (65, 50), (500, 64)])
def test_all_rewards_equal(L, monkeypatch, N, k):
    H, iters = 6, 2
    noise = _noise(N, 1, H, iters, 3)
    noise[:] = noise[:, :1]                              # every particle the same draws: all tied, the lowest indices win
    ref = _check_all_paths(L, monkeypatch, noise, O.pendulum_start_states(1), N, H, iters, k)
    np.testing.assert_array_equal(ref[5][0][0], np.arange(k))
    # a NaN state: every reward is the guard value -1e6
    bad = np.array([[np.nan, 0.0, 0.0]], F)
    ref = _check_all_paths(L, monkeypatch, _noise(N, 1, H, iters, 4), bad, N, H, iters, k)
    assert np.all(ref[6][0] == F(-1e6))
    np.testing.assert_array_equal(ref[5][0][0], np.arange(k))


# ------------------------------------------------------------------------------------------------
def _closed_loop(eng, steps, inject_at=(), L=None):
    s = O.pendulum_start_states(eng.A)
    out = []
    for t in range(steps):
        if t in inject_at:                               # the caller's own draws for this call: a launch, and the resident
            rng = np.random.default_rng(1000 + t)        # kernel that follows starts from another pointer
            eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack([O.truncated_normal_noise(rng, (eng.N, eng.A, eng.H, 1))
                                                             for _ in range(eng.iters)]).astype(F))
        a, s, r = eng.optimize(s, t, add_exploration_noise=(t % 5 == 2))
        if t in inject_at:
            eng.inject_noise(L.NOISE_TRUNC_NORMAL, None)
        out.append(np.concatenate([a.ravel(), s.ravel(), np.ravel(r)]))
    return np.stack(out)


@pytest.mark.parametrize("inject_at", [(), (3, 4, 11)])
def test_resident_hand_off_is_bit_identical_across_chunk_boundaries(L, monkeypatch, inject_at):
    steps = 20
    monkeypatch.setenv("BBMPC_LINGER_US", "0")
    e0 = _engine(L, 64, 8, 3, 8, seed=11)
    ref = _closed_loop(e0, steps, inject_at, L)
    assert e0.call_stats() == (0, steps)
    e0.close()
    monkeypatch.delenv("BBMPC_LINGER_US")
    e1 = _engine(L, 64, 8, 3, 8, seed=11)
    got = _closed_loop(e1, steps, inject_at, L)
    served, launched = e1.call_stats()
    e1.close()
    np.testing.assert_array_equal(got, ref)
    assert served + launched == steps
    # launches: call 0; every call with injected draws (the non-resident form) and the call after it (clearing the draws is
    # an entry point of its own, which ends a resident kernel).  Everything else rides the resident kernel.
    want_launched = 1 + len(set(inject_at) | set(t + 1 for t in inject_at))
    print("served %d launched %d (expected %d launched)" % (served, launched, want_launched))
    assert launched == want_launched and served == steps - want_launched
