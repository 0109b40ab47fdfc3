"""GPU tests of discounted, termination-aware returns (bbmpc_set_return_shaping, k_shaped_return) through the C ABI.

Against the statement (tests/return_shaping_util.py, float64) applied to the handle's own predict_trajectories states and
step rewards, at tests/reward_mlp_util's H-step tolerance (rtol 1e-3 + atol 1e-3 H).  The bound test is a discontinuity:
a candidate with any (t, i) within 1e-3 * max(1, |bound|) of an active bound is left out of the comparison, and at most
5 % may be.  Shapes: S = 3 / U = 1 (4-8-3, S % 4 != 0: scalar plane loads) and S = 20 / U = 6 (26-16-20: float4 plane
loads, the cheetah reward reads index 17); N = 37 (a partial wave) and 70 (two waves); A in {1, 3}; H in {1, 5}."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import bounds_util as B
from tests import nonfinite_util as NF
from tests import return_shaping_util as RS
from tests import reward_mlp_util as R
from tests import terminal_value_util as V

pytestmark = pytest.mark.gpu
F = np.float32
INF = np.inf


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _dynamics(S, U, hidden, seed=42):
    """a random model whose steps are a good fraction of the states' spread, so that rollouts cross a bound at every step"""
    dims = [S + U] + hidden + [S]
    ws, bs = O.make_mlp_params(dims, seed=seed)
    rng = np.random.default_rng(seed + 2)
    stats = [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F), rng.normal(0, 0.1, U).astype(F),
             rng.uniform(0.5, 1.5, U).astype(F), rng.normal(0, 0.05, S).astype(F), rng.uniform(0.3, 0.6, S).astype(F)]
    return ws, bs, [1] * len(hidden) + [0], stats


REWARD_NET = R.small_nets()[1]                                 # 7-20-1 over (s_t, a_t, s_{t+1}), S = 3, U = 1
VALUE_NETS = {3: V.small_nets()[1], 20: R.Net("v-20-16-1", 20, 6, 1, [16], ["tanh", None], True, 31)}
KINDS = ("pendulum", "pendulum-q1", "cheetah", "mlp")


def _engine(L, kind, A=1, H=5, opt=None, **kw):
    from blackbox_mpc_amd.engine import Engine
    S, U = (20, 6) if kind == "cheetah" else (3, 1)
    rew = {"pendulum": L.REW_PENDULUM, "pendulum-q1": L.REW_PENDULUM, "cheetah": L.REW_CHEETAH, "mlp": L.REW_MLP}[kind]
    if kind == "pendulum-q1":
        kw["quirks"] = kw.get("quirks", 0) | L.FIX_Q1_REWARD_ARG_ORDER
    eng = Engine(L.OPT_NONE if opt is None else opt, L.DYN_MLP, rew, [-1.0] * U, [1.0] * U, dim_s=S, num_agents=A, planning_horizon=H, **kw)
    eng.set_mlp(*_dynamics(S, U, [16] if S == 20 else [8]))
    if kind == "mlp":
        eng.set_reward_mlp(REWARD_NET.ws, REWARD_NET.bs, REWARD_NET.codes(), REWARD_NET.mask, REWARD_NET.stats)
    return eng


def _set_value(eng, w=0.75):
    net = VALUE_NETS[eng.S]
    eng.set_terminal_value_mlp(net.ws, net.bs, net.codes(), net.stats, w)
    return net, w


def _inputs(eng, N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0, 0.5, (eng.A, eng.S)).astype(F), rng.uniform(-1, 1, (N, eng.A, eng.H, eng.U)).astype(F)


def _reference(eng, state, seq):
    """the handle's own states [N, A, H, S] and step rewards [N, A, H] (predict_trajectories never reads the shaping)"""
    N, A, H, U = seq.shape
    rows_s = np.broadcast_to(state[None], (N, A, state.shape[1])).reshape(N * A, -1)
    states, rews = eng.predict_trajectories(rows_s, seq.reshape(N * A, H, U))
    return states.reshape(N, A, H, -1), rews.reshape(N, A, H)


def _box(states, H):
    """A bound from quantiles of the reference trajectories: `hi` on one coordinate at a percentile of that coordinate over
    all (n, a, t) -- the first (coordinate, percentile) for which candidates terminate at step 1, at step H and never, and
    at most 5 % of them come within the exclusion band of the bound.  Chosen from the reference trajectories alone."""
    S = states.shape[-1]
    lo = np.full(S, -INF, F)
    for q in sorted(range(30, 96), key=lambda p: (abs(p - 70), p)):           # the 70th percentile first, then its neighbours
        for i in range(S):
            hi = np.full(S, INF, F)
            hi[i] = F(np.percentile(states[..., i], q))
            _, T = RS.shaped_return(np.zeros(states.shape[:-1]), states, 1.0, None, hi)
            if (T == 1).any() and (T == 0).any() and (H == 1 or (T == H).any()) and RS.near_bound(states, lo, hi).mean() <= 0.05:
                return lo, hi, (i, q)
    raise AssertionError("no quantile bound splits these trajectories into step-1, step-H and never")


def _raises(L, code, fn):
    with pytest.raises(L.BBMPCError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    return str(ei.value)


def _tol(H):
    return dict(rtol=R.H_STEP_RTOL, atol=R.H_STEP_ATOL_PER_STEP * H)


# ---- 1. evaluate against the statement ---------------------------------------------------------------------------------------
# observed share of candidates left out as too close to the bound: 1.0 .. 4.8 % over these cases (printed per case; at N = 37,
# A = 1 one candidate is 2.7 %)
@pytest.mark.parametrize("with_value", [False, True], ids=["noV", "V"])
@pytest.mark.parametrize("N,A,H", [(70, 3, 5), (37, 1, 5), (37, 3, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_evaluate_against_the_statement(L, kind, N, A, H, with_value):
    eng = _engine(L, kind, A=A, H=H)
    for seed in range(100 + N + A + H, 100 + N + A + H + 8000, 1000):    # the first seed whose trajectories a quantile bound splits
        state, seq = _inputs(eng, N, seed)
        states, rews = _reference(eng, state, seq)
        try:
            _box(states, H)
            break
        except AssertionError:
            continue
    plain = eng.evaluate(state, seq)
    _raises(L, L.E_STATE, lambda: eng.termination_steps())                 # shaping is off
    vterm, w = None, 1.0
    if with_value:
        net, w = _set_value(eng)
        vterm = V.value(net, states[:, :, -1].reshape(N * A, -1)).reshape(N, A)
    lo, hi, (coord, q) = _box(states, H)
    near = RS.near_bound(states, lo, hi)
    print("%s N=%d A=%d H=%d: hi[%d] at the %dth percentile, %.1f %% of the candidates within the band" % (kind, N, A, H, coord, q, 100.0 * near.mean()))
    assert near.mean() <= 0.05
    for gamma in (1.0, 0.9):
        for c in (0.0, -5.0):
            eng.set_return_shaping(gamma, lo, hi, c)
            got = eng.evaluate(state, seq)
            T = eng.termination_steps()
            want, want_T = RS.shaped_return(rews, states, gamma, lo, hi, c, None, vterm, w)
            assert (want_T == 1).any() and (want_T == 0).any() and (H == 1 or (want_T == H).any())
            print("  gamma %.1f c %4.1f: max |R - statement| = %.3g" % (gamma, c, np.max(np.abs(got - want)[~near])))
            np.testing.assert_array_equal(T[~near], want_T[~near])
            np.testing.assert_allclose(got[~near], want[~near], **_tol(H))
            assert got.dtype == F and T.dtype == np.int32 and T.shape == (N, A)
    eng.set_return_shaping(1.0)                                # off, the value network (if any) stays: what the shaping moved
    assert np.max(np.abs(got - eng.evaluate(state, seq))) > 10 * R.H_STEP_ATOL_PER_STEP * H
    # both bounds at once on another coordinate, lo alone active there
    lo2 = lo.copy()
    lo2[(coord + 1) % eng.S] = F(np.percentile(states[..., (coord + 1) % eng.S], 25))
    near2 = RS.near_bound(states, lo2, hi)
    eng.set_return_shaping(0.9, lo2, hi, -5.0)
    got = eng.evaluate(state, seq)
    want, want_T = RS.shaped_return(rews, states, 0.9, lo2, hi, -5.0, None, vterm, w)
    np.testing.assert_array_equal(eng.termination_steps()[~near2], want_T[~near2])
    np.testing.assert_allclose(got[~near2], want[~near2], **_tol(H))


# ---- 2. identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_value", [False, True], ids=["noV", "V"])
@pytest.mark.parametrize("kind", KINDS)
def test_discount_one_without_bounds_is_the_unshaped_handle(L, kind, with_value):
    N, A, H = 37, 3, 5
    eng = _engine(L, kind, A=A, H=H)
    state, seq = _inputs(eng, N, 7)
    if with_value:
        _set_value(eng)
    before = eng.evaluate(state, seq)
    S = eng.S
    eng.set_return_shaping(1.0, np.full(S, -INF, F), np.full(S, INF, F), -5.0)       # on, and the identity
    same = eng.evaluate(state, seq)
    assert not eng.termination_steps().any()
    if kind == "mlp" and not with_value:                       # same step buffer, ascending sum, g = 1 exact
        np.testing.assert_array_equal(same.view(np.uint32), before.view(np.uint32))
    else:
        np.testing.assert_allclose(same, before, **_tol(H))
    eng.set_return_shaping(0.9)                                # a discount alone
    assert np.max(np.abs(eng.evaluate(state, seq) - before)) > 10 * R.H_STEP_ATOL_PER_STEP * H
    eng.set_return_shaping(1.0, None, None)                    # off: the routing and the bits of before
    np.testing.assert_array_equal(eng.evaluate(state, seq).view(np.uint32), before.view(np.uint32))
    _raises(L, L.E_STATE, lambda: eng.termination_steps())


# ---- 3. isolation --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum-q1", "cheetah", "mlp"])
def test_nan_actions_behind_the_terminal_step_are_not_read(L, kind):
    N, A, H = 37, 2, 5
    eng = _engine(L, kind, A=A, H=H)
    state, seq = _inputs(eng, N, 11)
    states, _ = _reference(eng, state, seq)
    lo, hi, _ = _box(states, H)
    near = RS.near_bound(states, lo, hi)
    _set_value(eng)
    eng.set_return_shaping(0.9, lo, hi, -5.0)
    clean, T = eng.evaluate(state, seq), eng.termination_steps()
    early = [(n, a) for n in range(N) for a in range(A) if 1 <= T[n, a] <= H - 2 and not near[n, a]]
    late = [(n, a) for n in range(N) for a in range(A) if (T[n, a] == 0 or T[n, a] >= 3) and not near[n, a]]
    assert len(early) >= 2 and len(late) >= 2
    behind, before = seq.copy(), seq.copy()
    for n, a in early:                                         # NaN in every action behind the terminal step
        behind[n, a, T[n, a]:] = np.nan
    got = eng.evaluate(state, behind)
    np.testing.assert_array_equal(got.view(np.uint32), clean.view(np.uint32))
    np.testing.assert_array_equal(eng.termination_steps(), T)
    assert np.all(np.isfinite(got))
    poisoned = set(late[::2])
    for n, a in poisoned:                                      # NaN in front of it: step 1 of a candidate that lives to step 3 at least
        before[n, a, 1, -1] = np.nan
    NF.check(clean, eng.evaluate(state, before), poisoned, "NaN before the terminal step")


# ---- 4. determinism and the agent split ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "cheetah", "mlp"])
def test_agent_split_and_repeat_give_equal_bits(L, kind):
    N, H = 70, 5
    eng = _engine(L, kind, A=4, H=H)
    state4, seq4 = _inputs(eng, N, 2)
    states, _ = _reference(eng, state4, seq4)
    lo, hi, _ = _box(states, H)
    _set_value(eng)
    eng.set_return_shaping(0.9, lo, hi, -5.0)
    full, T = eng.evaluate(state4, seq4), eng.termination_steps()
    np.testing.assert_array_equal(eng.evaluate(state4, seq4).view(np.uint32), full.view(np.uint32))
    np.testing.assert_array_equal(eng.termination_steps(), T)
    for off in (0, 2):
        half = _engine(L, kind, A=2, H=H, agent_offset=off, num_agents_global=4)
        _set_value(half)
        half.set_return_shaping(0.9, lo, hi, -5.0)
        got = half.evaluate(state4[off:off + 2], np.ascontiguousarray(seq4[:, off:off + 2]))
        np.testing.assert_array_equal(got.view(np.uint32), np.ascontiguousarray(full[:, off:off + 2]).view(np.uint32))
        np.testing.assert_array_equal(half.termination_steps(), T[:, off:off + 2])


# ---- 5. the optimizers -------------------------------------------------------------------------------------------------------------
OPTS = ("RS", "CEM", "PI2", "SPSA", "PSO", "CMA")
SPSA_C, SPSA_GAMMA = 1.5, 0.101                                # c large enough that mean +- c_k * delta leaves [-1, 1]


def _opt(L, name):
    return {"RS": L.OPT_RANDOM_SEARCH, "CEM": L.OPT_CEM, "PI2": L.OPT_PI2, "SPSA": L.OPT_SPSA, "PSO": L.OPT_PSO, "CMA": L.OPT_CMAES}[name]


def _control_step(L, kind, opt_name, shaping, state, lo, hi, trace=True):
    """one control step of a handle with a value network; candidates that leave the action bounds [-1, 1] on purpose"""
    N = {"SPSA": 4, "CMA": 16}.get(opt_name, 37)
    A, H, iters = 2, 5, 2
    kw = dict(A=A, H=H, opt=_opt(L, opt_name), population_size=N, max_iterations=iters, num_elite=4, seed=3)
    if opt_name == "CMA":
        kw["quirks"] = L.CMAES_PER_AGENT
    if opt_name == "SPSA":
        kw.update(spsa_c=SPSA_C, spsa_gamma=SPSA_GAMMA)
    eng = _engine(L, kind, **kw)
    _set_value(eng)
    if shaping:
        eng.set_return_shaping(0.9, lo, hi, -5.0)
    eng.set_trace(trace)
    if opt_name in ("CEM", "PI2"):
        eng.set_state("var0", np.ones((A, H, eng.U), F))       # unit variance on a range of 2: draws leave the bounds on both sides
    pos0 = eng.get_state("pos", (N, A, H, eng.U)) if opt_name == "PSO" else None
    mean0 = eng.get_state("prev_mean") if opt_name == "SPSA" else None
    out = eng.optimize(state)
    return eng, out, pos0, mean0


def _spsa_candidates(eng, L, it, mean_before):
    """SPSA's 2N candidates of iteration `it` as drawn, (+) then (-): mean +- c_k * delta, c_k = c / (it + 1)^gamma (spsa.py:70)"""
    ck = F(SPSA_C) / F((it + 1.0) ** SPSA_GAMMA)
    delta = eng.get_trace(it, L.TRACE_SAMPLES)                 # [N, A, H, U]
    return np.concatenate([mean_before[None] + ck * delta, mean_before[None] - ck * delta], 0).astype(F)


@pytest.mark.parametrize("kind", ["pendulum", "mlp"])
@pytest.mark.parametrize("opt_name", OPTS)
def test_control_steps_score_their_candidates_with_the_shaped_return(L, opt_name, kind):
    """Traced rewards of a control step = `evaluate` of the candidates on the same handle - bound penalty, under action bounds
    that the draws leave.  The candidates: RandomSearch, CEM, PI2 and CMA-ES trace theirs (clipped); SPSA's are rebuilt from
    the traced iterate and perturbation; PSO traces none and moves its particles before the host can read them, so its first
    iteration alone is checked, from the positions read before the step.  The penalty sum (x - clip(x))^2 is known where the
    drawn candidates are (SPSA, PSO); CEM and RandomSearch charge none.  For PI2 and CMA-ES only the clipped candidates are
    traced: in the first iteration, where a shaped and an unshaped handle of one seed draw the same candidates, the penalty is
    what the unshaped handle charged (its evaluate - its traced reward); afterwards candidates strictly inside the bounds
    are compared exactly and the others must not score above their evaluate."""
    A, H = 2, 5
    probe = _engine(L, kind, A=A, H=H)
    state, seq = _inputs(probe, 64, 3)
    states, _ = _reference(probe, state, seq)
    lo, hi, _ = _box(states, H)
    eng, _, pos0, mean0 = _control_step(L, kind, opt_name, True, state, lo, hi)
    ref, _, _, _ = _control_step(L, kind, opt_name, False, state, lo, hi)
    n_it = 1 if opt_name in ("RS", "PSO") else eng.iters
    tol, clipped_seen, differs = _tol(H), 0, False
    for it in range(n_it):
        r_s, r_p = eng.get_trace(it, L.TRACE_REWARDS), ref.get_trace(it, L.TRACE_REWARDS)
        pen = None
        if opt_name == "SPSA":
            mean = mean0 if it == 0 else eng.get_trace(it - 1, L.TRACE_MEAN)
            raw = _spsa_candidates(eng, L, it, mean)
        elif opt_name == "PSO":
            raw = pos0
        else:
            raw = None
        if raw is not None:
            x = np.clip(raw, -1.0, 1.0).astype(F)
            pen = np.sum((raw.astype(np.float64) - x) ** 2, axis=(2, 3))
        else:
            x = eng.get_trace(it, L.TRACE_SAMPLES)
            if opt_name in ("RS", "CEM"):
                pen = np.zeros(r_s.shape)
            elif it == 0:                                      # same seed, same first draws: the unshaped handle's own penalty
                np.testing.assert_array_equal(x, ref.get_trace(0, L.TRACE_SAMPLES))
                pen = ref.evaluate(state, x).astype(np.float64) - r_p
                assert np.all(pen > -(tol["atol"] + tol["rtol"] * np.abs(r_p)))
        again = eng.evaluate(state, x).astype(np.float64)
        on_bound = np.any(np.abs(x) >= 1.0, axis=(2, 3))
        clipped_seen += int(on_bound.sum())
        if pen is not None:
            np.testing.assert_allclose(r_s, again - pen, err_msg="%s iteration %d" % (opt_name, it), **tol)
        else:
            np.testing.assert_allclose(r_s[~on_bound], again[~on_bound], err_msg="%s iteration %d" % (opt_name, it), **tol)
            assert np.all(r_s[on_bound] <= again[on_bound] + tol["atol"] + tol["rtol"] * np.abs(again[on_bound]))
        differs |= bool(np.any(np.abs(again - ref.evaluate(state, x)) > 10 * R.H_STEP_ATOL_PER_STEP * H))
    assert differs                                             # the shaped scores are not the unshaped ones
    if opt_name in ("PI2", "SPSA", "CMA"):                     # (RandomSearch and CEM draw inside the bounds, PSO starts inside them)
        assert clipped_seen > 0                                # clipping and the penalty took part
    T = eng.termination_steps()                                # of the last rollout, whatever its population
    assert T.shape[1] == A and T.min() >= 0 and T.max() <= H


@pytest.mark.parametrize("kind", ["pendulum", "cheetah"])
def test_cmaes_scores_the_clipped_candidates_with_the_trace_off(L, kind):
    """CMA-ES writes its clipped candidates back only when somebody reads them; k_shaped_return does (a_t of a built-in reward).
    A control step with the trace off equals the traced one bit for bit: action, next state, reward, and T."""
    A, H = 2, 5
    probe = _engine(L, kind, A=A, H=H)
    state, seq = _inputs(probe, 64, 3)
    states, _ = _reference(probe, state, seq)
    lo, hi, _ = _box(states, H)
    traced, out_t, _, _ = _control_step(L, kind, "CMA", True, state, lo, hi, trace=True)
    plain, out_p, _, _ = _control_step(L, kind, "CMA", True, state, lo, hi, trace=False)
    x = traced.get_trace(traced.iters - 1, L.TRACE_SAMPLES)
    assert np.any(np.abs(x) >= 1.0)                            # draws left the bounds
    for got, want in zip(out_p, out_t):
        np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(plain.termination_steps(), traced.termination_steps())


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_error_codes(L):
    from blackbox_mpc_amd.engine import Engine
    from tests import particle_user_reward_util as RU
    N, A, H = 8, 1, 3
    eng = _engine(L, "pendulum", A=A, H=H)
    state, seq = _inputs(eng, N, 0)
    plain = eng.evaluate(state, seq)
    lo, hi = np.array([-INF, -INF, -0.2], F), np.array([INF, INF, 0.2], F)

    def usable(e, want):
        np.testing.assert_array_equal(e.evaluate(state, seq), want)

    for bad in (0.0, -0.5, 1.5, np.nan, INF):
        assert "discount" in _raises(L, L.E_INVALID, lambda: eng.set_return_shaping(bad, lo, hi))
    assert "NaN" in _raises(L, L.E_INVALID, lambda: eng.set_return_shaping(0.9, np.array([np.nan, 0, 0], F), hi))
    assert "exceeds" in _raises(L, L.E_INVALID, lambda: eng.set_return_shaping(0.9, np.array([0, 0, 1.0], F), hi))
    for bad in (np.nan, INF, -INF):
        assert "terminal_reward" in _raises(L, L.E_INVALID, lambda: eng.set_return_shaping(0.9, lo, hi, bad))
    usable(eng, plain)
    _raises(L, L.E_STATE, lambda: eng.termination_steps())
    # particles, either order
    eng.set_particles(4, np.zeros(3, F), 0.0)
    assert "particles" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_return_shaping(0.9, lo, hi))
    eng.set_particles(0)
    usable(eng, plain)
    eng.set_return_shaping(0.9, lo, hi, -5.0)
    _raises(L, L.E_STATE, lambda: eng.termination_steps())                 # on, nothing rolled out yet
    shaped = eng.evaluate(state, seq)
    assert np.max(np.abs(shaped - plain)) > 0.1
    assert L.lib.bbmpc_get_termination_steps(eng._h, None, N * A) == L.E_INVALID
    _raises(L, L.E_INVALID, lambda: eng.termination_steps(N + 1))
    assert "bbmpc_set_return_shaping" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_particles(4, np.zeros(3, F), 0.0))
    usable(eng, shaped)
    # an inverse target transform, either order
    assert "bbmpc_set_return_shaping" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_inverse_transform_source(B.XFORM_SOURCE))
    usable(eng, shaped)
    _raises(L, L.E_INVALID, lambda: eng.set_return_shaping(0.0, lo, hi))   # a refused replacement keeps the old setting
    usable(eng, shaped)
    eng.set_return_shaping(1.0)
    eng.set_inverse_transform_source(B.XFORM_SOURCE)
    with_x = eng.evaluate(state, seq)
    assert "transform" in _raises(L, L.E_UNSUPPORTED, lambda: eng.set_return_shaping(0.9, lo, hi))
    usable(eng, with_x)
    # gradient refinement and the gradient calls
    cem = _engine(L, "mlp", A=A, H=H, opt=L.OPT_CEM, population_size=16, max_iterations=1, num_elite=4)
    rows = np.ascontiguousarray(np.broadcast_to(state, (N, 3)))
    ret, _ = cem.plan_gradient(rows, seq[:, 0])
    cem.set_grad_refine(2, 0.05, "adam", 0)
    assert "bbmpc_set_grad_refine" in _raises(L, L.E_UNSUPPORTED, lambda: cem.set_return_shaping(0.9, lo, hi))
    cem.set_grad_refine(0, 0.05, "adam", 0)
    cem.set_return_shaping(0.9, lo, hi)
    for fn in (lambda: cem.set_grad_refine(2, 0.05, "adam", 0), lambda: cem.plan_gradient(rows, seq[:, 0]),
               lambda: cem.refine_plans(rows, seq[:, 0], 2, 0.05)):
        assert "bbmpc_set_return_shaping" in _raises(L, L.E_UNSUPPORTED, fn)
    cem.set_return_shaping(1.0)
    np.testing.assert_array_equal(cem.plan_gradient(rows, seq[:, 0])[0], ret)
    # rewards and dynamics without a shaped form
    user = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_USER, [-1.0], [1.0], dim_s=3, num_agents=A, planning_horizon=H)
    user.set_mlp(*_dynamics(3, 1, [8]))
    user.set_reward_source(RU.MIXED_REWARD)
    scored = user.evaluate(state, seq)
    assert "BBMPC_REW_USER" in _raises(L, L.E_UNSUPPORTED, lambda: user.set_return_shaping(0.9, lo, hi))
    usable(user, scored)
    pend = Engine(L.OPT_NONE, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H)
    p0 = pend.evaluate(state, seq)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: pend.set_return_shaping(0.9, lo, hi))
    usable(pend, p0)
    pend.set_return_shaping(1.0)                               # off is always allowed
    udyn = Engine(L.OPT_NONE, L.DYN_USER, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H)
    assert "BBMPC_DYN_MLP" in _raises(L, L.E_UNSUPPORTED, lambda: udyn.set_return_shaping(0.9, lo, hi))


# ---- 7. the Python layer ---------------------------------------------------------------------------------------------------------
def test_python_layer_plans_with_the_box_and_reuploads_changed_bounds(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.policies.mpc_policy import MPCPolicy
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    from blackbox_mpc_amd.utils.rollouts import ModelEnvironment
    from blackbox_mpc_amd.utils.termination import StateBoxTermination
    act_space, obs_space = Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])
    A, H, N = 3, 5, 37
    ws, bs, acts, stats = _dynamics(3, 1, [8])
    dyn = DeterministicMLP(layers=[4, 8, 3], activation_functions=["tanh", None], seed=0)
    dyn.set_weights(ws, bs)
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=dyn)
    handler.set_normalization_stats(*stats)
    start = np.random.default_rng(5).normal(0, 0.5, (A, 3)).astype(F)
    seq = np.random.default_rng(0).uniform(-2, 2, (N, A, H, 1)).astype(F)
    plain = DeterministicTrajectoryEvaluator(pendulum_reward_function, handler)
    rows_s = np.broadcast_to(start[None], (N, A, 3)).reshape(N * A, 3)
    states, rews = plain.predict_trajectories(rows_s, seq.reshape(N * A, H, 1))
    states, rews = states.reshape(N, A, H, 3), rews.reshape(N, A, H)
    lo, hi, (coord, _) = _box(states, H)
    box = StateBoxTermination(lo, hi, terminal_reward=-5.0)
    policy = MPCPolicy(reward_function=pendulum_reward_function, env_action_space=act_space, env_observation_space=obs_space,
                       dynamics_handler=handler, optimizer_name="CEM", num_agents=A, planning_horizon=H, population_size=64, num_elite=8,
                       max_iterations=2, seed=4, discount=0.9, termination=box)
    a1, n1, r1 = policy.act(start, 0)
    # ... equals the engine-level result: a handle configured by hand, same optimizer arguments
    from blackbox_mpc_amd.engine import Engine
    hand = Engine(L.OPT_CEM, L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H, population_size=64,
                  max_iterations=2, num_elite=8, seed=4)
    hand.set_mlp(dyn.weights, dyn.biases, dyn.activation_codes, handler.normalization_stats())
    hand.set_return_shaping(0.9, lo, hi, -5.0)
    a2, n2, r2 = hand.optimize(start)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(n1, n2)
    ev = policy._trajectory_evaluator

    def check():
        near = RS.near_bound(states, box.low, box.high)
        want, want_T = RS.shaped_return(rews, states, 0.9, box.low, box.high, box.terminal_reward)
        got = ev(start, seq)
        np.testing.assert_allclose(got[~near], want[~near], **_tol(H))
        return got
    first = check()
    done = ModelEnvironment(ev, start).step(np.zeros((A, 1), F))[2]
    np.testing.assert_array_equal(done, box(ev.predict_next_state(start, np.zeros((A, 1), F))))
    hi2 = hi.copy()
    hi2[coord] = F(np.percentile(states[..., coord], 40))
    v = box._version
    box.set_bounds(lo, hi2)
    assert box._version > v
    policy.act(start, 1)                                       # the optimizer's engine uploads the new box before it plans
    assert policy._optimizer._engine._shaping_version[2] == box._version
    second = check()
    assert np.max(np.abs(second - first)) > 0.05
