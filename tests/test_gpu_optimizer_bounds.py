"""Every optimizer under asymmetric, per-dimension action bounds, by value against oracle_np, on every path that forms
candidates from the bounds.  The inputs (bound sets, draws, start states) are those of tests/bounds_util.py; that they make
the oracle clip on both sides, pay penalties and constrain the variance on either side of the midpoint is asserted on the
oracle alone in tests/test_bounds_cpu.py.

How a case is compared.  Two engines of one configuration get the same states and draws: a TRACED one (set_trace, which
routes a handle to the launch paths that keep every iteration) and a PLAIN one on the path the case is about, asserted
through _assert_path / get_profile.  The oracle runs in lock-step with the traced engine's per-iteration trace -- the
existing recipes: the device's elite set after a tie check (CEM, as _cem_lockstep / _lockstep_select), the device's rewards
after a tolerance check (PI2, PSO: rewards_override), the device's eigen-system and elite order (CMA-ES: eig / forced_order
as test_cmaes_coupled_lockstep) -- and BOTH engines' actions, warm starts and optimizer state are then held to that oracle
at the lock-step tolerances.  The resident kernel and the untraced CMA-ES kernels cannot be traced; they compute the same
bits as their traced twins (tests/test_gpu_resident.py, tests/test_gpu_cmaes.py), which is what makes the twin's lock-step
valid for them.  Draws are injected, or (mode "production") the engine's own, read back through dump_noise.

Tolerances are the existing ones for the same quantities: candidates 1e-5 and exactly the bound where the oracle clips
(CMA-ES 2e-5 as test_cmaes_coupled_lockstep); pendulum rewards R_RTOL 2e-4 / R_ATOL 2e-3, learned rtol 1e-3 / atol 1e-3 H;
CEM mean / var 2e-5 (pendulum) and 1e-4 (learned); PI2 mean 2e-5 in lock-step; SPSA 1e-4; PSO state 2e-5."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import bounds_util as B
from tests.parity_util import assert_cheetah_rewards, assert_pendulum_rewards, cheetah_threshold_margin
from tests import tail_util as T
from tests.tail_util import ACT, MLP_SHAPES
from tests.test_gpu_control_step_tail import PENDULUM_TAILS, _assert_path, _close, _opt, _set_path

pytestmark = pytest.mark.gpu
F = np.float32
N, H, K, ITERS, STEPS = B.N, B.H, B.K, B.ITERS, B.STEPS
SEED = 0x0B0D5EED12345678
R_RTOL, R_ATOL = 2e-4, 2e-3                    # pendulum H-step rewards (test_gpu_pendulum.py)
M_RTOL, M_ATOL = 1e-3, 1e-3 * H                # learned-model H-step rewards (test_gpu_mlp.py)


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _base(opt_name):
    return opt_name.replace("-reset", "")


# the other kernels that form candidates from the bounds: variant -> (problem of bounds_util, environment, profile name;
# a trailing * = "contains")
VARIANTS = {
    "pair0": ("S20-U6-h200", {"BBMPC_MLP_Q4": "0", "BBMPC_MLP_PAIR": "0"}, "k_rollout_mlp_pair"),
    "pair1": ("S20-U6-h200", {"BBMPC_MLP_Q4": "0", "BBMPC_MLP_PAIR": "1"}, "k_rollout_mlp_pair"),
    "wave": ("S3-U2-h16", {"BBMPC_MLP_W4": "0"}, "k_rollout_mlp_wave"),
    "generic": ("S3-U2-h16", {"BBMPC_MLP_WAVE": "0", "BBMPC_MLP_W4": "0"}, "k_rollout_mlp"),
    "generic-U64": ("S64-U64-h96", {"BBMPC_MLP_WAVE": "0", "BBMPC_MLP_W4": "0"}, "k_rollout_mlp"),
    "xform": ("xform-U2", {}, "bbmpc_mlp_xform_rollout(hiprtc)"),
    "user": ("user-U2", {}, "user*"),
    "particles-pendulum": ("asym", {}, "k_rollout_pendulum_particles"),
    "particles-mlp": ("S20-U6-h200", {}, "k_rollout_mlp_particles"),
    "corr": ("corr-U2", {}, "k_rollout_mlp*"),
}


def _kernel_ok(name, want):
    return (want[:-1] in name) if want.endswith("*") else name == want


class Problem:
    """bounds, oracle evaluator, start states (all from bounds_util.problem, as tests/test_bounds_cpu.py) and the engine
    factory of a case"""

    def __init__(self, name, A, variant=None):
        self.name, self.A, self.variant = name, A, variant
        self.ev, self.lo, self.hi, self.states, self.reward = B.problem(name, A)
        self.pendulum = name in B.PENDULUM_SETS
        self.analytic = self.pendulum or name == "user-U2"      # no learned model: the pendulum tests' tolerances
        self.shape = None if self.analytic else ("S3-U2-h16" if name in ("xform-U2", "corr-U2") else name)
        self.S, self.U = self.states.shape[-1], self.lo.shape[0]
        self.mix = B.case_mix(name)

    def engine(self, L, opt_name, **kw):
        from blackbox_mpc_amd.engine import Engine
        opt, quirks, _ = _opt(L, _base(opt_name))
        args = dict(dim_s=self.S, num_agents=self.A, planning_horizon=H, population_size=N, max_iterations=ITERS, num_elite=K,
                    seed=SEED, quirks=quirks)
        args.update(kw)
        if self.pendulum:
            eng = Engine(opt, L.DYN_PENDULUM, L.REW_PENDULUM, self.lo, self.hi, **args)
        elif self.name == "user-U2":
            eng = Engine(opt, L.DYN_USER, L.REW_USER, self.lo, self.hi, **args)
            eng.set_dynamics_source(T.LINEAR_DYNAMICS)
            eng.set_reward_source(T.INTENDED_PENDULUM_REWARD)
        else:
            dims, acts, S, U, reward = MLP_SHAPES[self.shape]
            ws, bs, stats, _ = T.net(self.shape, True)
            eng = Engine(opt, L.DYN_MLP, L.REW_CHEETAH if reward == "cheetah" else L.REW_PENDULUM, self.lo, self.hi, **args)
            eng.set_mlp(ws, bs, [ACT[a] for a in acts], stats)
        if self.name == "xform-U2":
            eng.set_inverse_transform_source(B.XFORM_SOURCE)
        if self.variant in ("particles-pendulum", "particles-mlp"):
            # sigma = 0: every particle is the deterministic rollout, the score its mean -- the oracle's deterministic evaluator
            eng.set_particles(2, np.zeros(self.S, F), 0.0)
        if self.mix is not None:
            eng.set_sampling_correlation(self.mix)
        return eng

    def check_rewards(self, got, want, state, seq, what):
        """H-step rewards (bound penalty included on both sides) of candidates `seq` (None: not at hand)"""
        if self.pendulum and seq is not None:
            assert_pendulum_rewards(got, want, state, seq, R_RTOL, R_ATOL, what=what)
        elif self.analytic:
            np.testing.assert_allclose(got, want, rtol=R_RTOL, atol=R_ATOL, err_msg=what)
        elif self.reward == "cheetah":
            margin = (lambda: cheetah_threshold_margin(self.ev, state, seq)) if seq is not None else None
            assert_cheetah_rewards(got, want, M_RTOL, M_ATOL, what=what, horizon=H, margin=margin)
        else:
            np.testing.assert_allclose(got, want, rtol=M_RTOL, atol=M_ATOL, err_msg=what)

    def tie(self, kth):
        return (R_ATOL + R_RTOL * abs(kth)) if self.analytic else 2 * (M_ATOL + M_RTOL * abs(kth))

    def mean_atol(self):
        return 2e-5 if self.analytic else 1e-4


# ---- draws -----------------------------------------------------------------------------------------------------------
def _inject(L, eng, opt_name, noise):
    b = _base(opt_name)
    if b == "RS":
        eng.inject_noise(L.NOISE_UNIFORM, noise["uniform"])
    elif b in ("CEM", "CEM-warm", "PI2"):
        eng.inject_noise(L.NOISE_TRUNC_NORMAL, np.stack(noise["trunc"]))
    elif b == "SPSA":
        eng.inject_noise(L.NOISE_RADEMACHER, np.stack(noise["rademacher"]))
    elif b == "PSO":
        eng.inject_noise(L.NOISE_PSO_SCALARS, noise["normal2"])
        eng.inject_noise(L.NOISE_PSO_RESEED_TRUNC, noise["trunc"])
        eng.inject_noise(L.NOISE_PSO_RESEED_UNIFORM, noise["uniform"])
    else:
        eng.inject_noise(L.NOISE_NORMAL, np.stack(noise["normal"]))


def _production(L, eng, opt_name, step, A, U):
    """the engine's own draws of a control step (dump_noise: the documented Philox scheme), in the oracle's layout"""
    shape = (N, A, H, U)
    d = lambda kind, it: eng.dump_noise(kind, step, it, shape)
    b = _base(opt_name)
    if b == "RS":
        return {"uniform": d(L.NOISE_UNIFORM, 0)}
    if b in ("CEM", "CEM-warm", "PI2"):
        return {"trunc": [d(L.NOISE_TRUNC_NORMAL, it) for it in range(ITERS)]}
    if b == "SPSA":
        return {"rademacher": [d(L.NOISE_RADEMACHER, it) for it in range(ITERS)]}
    if b == "PSO":
        return {"normal2": np.stack([eng.dump_noise(L.NOISE_PSO_SCALARS, step, it, (2,)) for it in range(ITERS)]),
                "trunc": d(L.NOISE_PSO_RESEED_TRUNC, 0), "uniform": d(L.NOISE_PSO_RESEED_UNIFORM, 0)}
    return {"normal": [d(L.NOISE_NORMAL, it) for it in range(ITERS)]}


# ---- lock-step hooks + per-iteration comparisons of the traced engine ----------------------------------------------
def _groups(opt_name, A):
    return list(range(A)) if opt_name == "CMA-pa" else [None]


def _lock(L, P, eng, r, state, what):
    """the hooks Runner.step hands to the oracle, built from the traced engine's last control step"""
    b, A = r.name, P.A
    hip_r = [eng.get_trace(it, L.TRACE_REWARDS) for it in range(1 if b == "RS" else ITERS)]
    if b in ("CEM", "CEM-warm"):
        hip_el = [eng.get_trace(it, L.TRACE_ELITES) for it in range(ITERS)]

        def select(it, r_o, own):
            P.check_rewards(hip_r[it], r_o, state, eng.get_trace(it, L.TRACE_SAMPLES), "%s it %d" % (what, it))
            for a in range(A):
                he = hip_el[it][a]
                if set(own[a]) != set(he):
                    kth = np.sort(r_o[:, a])[::-1][K - 1]
                    for n in set(own[a]) ^ set(he):
                        assert abs(r_o[n, a] - kth) <= P.tie(kth), "%s: elite sets differ beyond the tie tolerance (it %d agent %d)" % (what, it, a)
                np.testing.assert_array_equal(he, O.topk_desc(hip_r[it][:, a], K))
            return hip_el[it]
        return dict(forced_elites=select)
    if b in ("PI2", "PSO", "PSO-reset"):
        def lock(it, r_o):
            # the candidates these rewards belong to: PI2's traced samples, the oracle's own clipped positions for PSO
            seq = eng.get_trace(it, L.TRACE_SAMPLES) if b == "PI2" else np.clip(r._sink[-1], P.lo, P.hi)
            P.check_rewards(hip_r[it], r_o, state, seq, "%s it %d" % (what, it))
            return hip_r[it]
        return dict(rewards_override=lock)
    if b in ("CMA", "CMA-pa"):
        per = b == "CMA-pa"
        Ag = 1 if per else A
        Bs = [eng.get_trace(it, L.TRACE_CMA_B) for it in range(ITERS)]
        Ds = [eng.get_trace(it, L.TRACE_CMA_D) for it in range(ITERS)]
        els = [eng.get_trace(it, L.TRACE_ELITES) for it in range(ITERS)]
        eigs, orders = [], []
        for g in range(A if per else 1):
            eigs.append([((Ds[it][g].astype(np.float64) ** 2).astype(F), Bs[it][g]) for it in range(ITERS)])

            def order(it, rsum, own, g=g):
                hr = hip_r[it][:, g] if per else hip_r[it].sum(axis=1, dtype=F)
                rt, at = (R_RTOL, R_ATOL * Ag) if P.analytic else (M_RTOL, M_ATOL * Ag)
                np.testing.assert_allclose(hr, rsum, rtol=rt, atol=at, err_msg="%s it %d" % (what, it))
                ho = els[it][g]
                np.testing.assert_array_equal(ho, O.topk_desc(hr, K))
                if not np.array_equal(own[:K], ho):             # only near-ties may swap
                    for a_, b_ in zip(own[:K], ho):
                        assert abs(rsum[a_] - rsum[b_]) <= at + rt * abs(rsum[a_]), "%s it %d: elite order differs beyond a tie" % (what, it)
                return ho
            orders.append(order)
        return dict(eig=eigs, forced_order=orders) if per else dict(eig=eigs[0], forced_order=orders[0])
    return {}


def _check_trace(L, P, eng, r, state, what, cover):
    """the traced engine's iterations against the (lock-stepped) oracle's; cover += candidates (at hi, at lo, inside)"""
    b, A, lo, hi = r.name, P.A, P.lo, P.hi
    tr, clips = r.opt.trace, r.clips[-1]
    if b == "RS":
        got = eng.get_trace(0, L.TRACE_SAMPLES)
        cover += np.array(B.check_candidates(got, tr[0]["samples"], lo, hi, 1e-5, what=what))
        hip_r = eng.get_trace(0, L.TRACE_REWARDS)
        P.check_rewards(hip_r, tr[0]["rewards"], state, got, what)
        best = eng.get_trace(0, L.TRACE_ELITES)
        np.testing.assert_array_equal(best, np.argmax(hip_r, axis=0))
        for a in range(A):                              # argmax may differ only between near-tied maxima
            top = tr[0]["rewards"][:, a].max()
            assert tr[0]["rewards"][best[a], a] >= top - 2 * P.tie(top), what
        return tr[0]["samples"][best, np.arange(A), 0, :]                  # the action the device's argmax stands for
    for it in range(ITERS):
        w = "%s it %d" % (what, it)
        if b in ("CEM", "CEM-warm"):
            raw = clips[it] if P.mix is not None else None              # (correlated CEM clips its mixed draws: correlated_util.py)
            cover += np.array(B.check_candidates(eng.get_trace(it, L.TRACE_SAMPLES), tr[it]["samples"], lo, hi, 1e-5, raw=raw, what=w))
            np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), tr[it]["mean"], rtol=0, atol=P.mean_atol(), err_msg=w)
            np.testing.assert_allclose(eng.get_trace(it, L.TRACE_VAR), tr[it]["var"], rtol=1e-5 if P.analytic else 1e-4, atol=P.mean_atol(), err_msg=w)
        elif b == "PI2":
            cover += np.array(B.check_candidates(eng.get_trace(it, L.TRACE_SAMPLES), tr[it]["samples"], lo, hi, 1e-5, raw=clips[it], what=w))
            np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), tr[it]["mean"], rtol=0, atol=2e-5, err_msg=w)
        elif b == "SPSA":
            hip_r = eng.get_trace(it, L.TRACE_REWARDS)
            P.check_rewards(hip_r[:N], tr[it]["rewards_plus"], state, np.clip(clips[3 * it], lo, hi), w + " plus")
            P.check_rewards(hip_r[N:], tr[it]["rewards_minus"], state, np.clip(clips[3 * it + 1], lo, hi), w + " minus")
            cover += np.array(B.check_candidates(eng.get_trace(it, L.TRACE_MEAN), tr[it]["solution"], lo, hi, 1e-4, raw=clips[3 * it + 2], what=w))
            # The device keeps no trace of SPSA's two perturbed candidates, the only place where its clip and penalty fire
            # under these sets: they are compared through their rewards alone (the penalty of a candidate clipped against the
            # wrong bound is off by far more than the reward tolerance, but a wrong index shows only that indirectly).  What is
            # asserted here: in every dimension narrower than 2 c_0 the rewards just compared include rows with a penalty
            if P.name not in B.SPSA_OUT_OF_REACH:
                narrow = (hi.astype(np.float64) - lo.astype(np.float64)) < B.SPSA_REACH
                for half in (0, 1):
                    pen = B.clip_coverage([clips[3 * it + half]], lo, hi)["penalised"]
                    assert narrow.any() and np.all(pen[narrow] >= 1), (w, pen)
        elif b in ("PSO", "PSO-reset"):
            np.testing.assert_array_equal(eng.get_trace(it, L.TRACE_ELITES), tr[it]["gbest_idx"], err_msg=w)
            if b == "PSO":
                # quirk Q4: without reset() pbest = 0 and pbest_r = 0 come from the constructor, every (negative) reward loses
                # against 0 (pso.py:84), so gbest -- and the action -- is the all-zero pbest, OUTSIDE bounds that exclude 0
                np.testing.assert_allclose(eng.get_trace(it, L.TRACE_MEAN), tr[it]["gbest"], rtol=0, atol=2e-5, err_msg=w)
            else:
                cover += np.array(B.check_candidates(eng.get_trace(it, L.TRACE_MEAN), tr[it]["gbest"], lo, hi, 2e-5, what=w))
        else:
            got, hip_r, hip_m = eng.get_trace(it, L.TRACE_SAMPLES), eng.get_trace(it, L.TRACE_REWARDS), eng.get_trace(it, L.TRACE_MEAN)
            for g in _groups(b, A):
                o = r.opts[g or 0]
                sl = slice(None) if g is None else slice(g, g + 1)
                raw = r.clips[-1][(g or 0) * ITERS + it]
                cover += np.array(B.check_candidates(got[:, sl], o.trace[it]["samples"], lo, hi, 2e-5, raw=raw, what=w))
                P.check_rewards(hip_r[:, sl], o.trace[it]["rewards"], state[sl], got[:, sl], w)
                np.testing.assert_allclose(hip_m[sl].reshape(-1), o.trace[it]["m"], rtol=0, atol=2e-5, err_msg=w)
    return None


def _snapshot(r):
    """what the oracle leaves behind a control step: the warm start / mean and the optimizer state the device exposes"""
    o, b = r.opt, r.name
    s = {}
    if r.prev_mean() is not None:
        s["prev_mean"] = r.prev_mean().copy()
    if b in ("CEM", "CEM-warm", "PI2"):
        s["mean"] = o.trace[-1]["mean"].copy()
    if b == "SPSA":
        s["mean"] = o.trace[-1]["solution"].copy()
    if b in ("PSO", "PSO-reset"):
        s.update(pos=o.pos.copy(), vel=o.vel.copy(), pbest=o.pbest.copy(), pbest_r=o.pbest_r.copy(), gbest=o.gbest.copy(), gbest_r=o.gbest_r.copy())
    if b in ("CMA", "CMA-pa"):
        for name in ("m", "sigma", "p_sigma", "p_C"):
            s[name] = np.concatenate([getattr(q, name) for q in r.opts])
        s["C"] = np.stack([q.C for q in r.opts])
    return s


def _check_state(P, eng, r, snap, what):
    b, A, U = r.name, P.A, P.U
    at = 1e-4 if b == "SPSA" else (2e-5 if b == "PI2" else P.mean_atol())
    for name in ("prev_mean", "mean"):
        if name in snap:
            np.testing.assert_allclose(eng.get_state(name), snap[name], rtol=0, atol=at, err_msg="%s %s" % (what, name))
    if b in ("PSO", "PSO-reset"):                        # as _check_pso_state (test_gpu_spsa_pso.py), U > 1 included
        for name in ("pos", "vel", "pbest"):
            got = eng.get_state(name, (N, A, H, U))
            np.testing.assert_allclose(got, snap[name], rtol=0, atol=2e-5, err_msg="%s %s" % (what, name))
        np.testing.assert_array_equal(eng.get_state("pbest_r", (N, A)), snap["pbest_r"], err_msg=what)      # all -inf after a re-seed
        np.testing.assert_array_equal(eng.get_state("gbest_r", (A,)), snap["gbest_r"], err_msg=what)
        np.testing.assert_allclose(eng.get_state("gbest"), snap["gbest"], rtol=0, atol=2e-5, err_msg=what + " gbest")
    if b in ("CMA", "CMA-pa"):                           # the tolerances of test_cmaes_coupled_lockstep
        G = A if b == "CMA-pa" else 1
        n = H * U * (1 if b == "CMA-pa" else A)
        g = lambda name: eng.get_state(name, (G * n,))
        np.testing.assert_allclose(g("m"), snap["m"], rtol=0, atol=2e-5, err_msg=what + " m")
        np.testing.assert_allclose(g("sigma"), snap["sigma"], rtol=2e-5, atol=1e-6, err_msg=what + " sigma")
        np.testing.assert_allclose(g("p_sigma"), snap["p_sigma"], rtol=1e-4, atol=2e-5, err_msg=what + " p_sigma")
        np.testing.assert_allclose(g("p_C"), snap["p_C"], rtol=1e-4, atol=2e-5, err_msg=what + " p_C")
        np.testing.assert_allclose(eng.get_state("C", (G, n, n)), snap["C"], rtol=1e-4, atol=2e-5, err_msg=what + " C")


def _act_atol(P, b):
    return {"RS": 1e-5, "SPSA": 1e-4, "PI2": 2e-5, "PSO": 2e-5, "PSO-reset": 2e-5, "CMA": 2e-5, "CMA-pa": 2e-5}.get(b, P.mean_atol())


def _check_step_outputs(P, b, out, act_o, state, what):
    act, nxt, rew = out
    np.testing.assert_allclose(act, act_o, rtol=0, atol=_act_atol(P, b), err_msg=what + " action")
    if b != "PSO":                                       # (quirk Q4, see _check_trace: the un-reset swarm's action is its all-zero pbest)
        assert np.all(act >= P.lo) and np.all(act <= P.hi), what
    nxt_o = P.ev.predict_next_state(state, act)          # the tail: the model step of the engine's own action
    rt, at, rr, ra = (1e-5, 1e-5, 1e-5, 1e-5) if P.analytic else (2e-5, 2e-5, 1e-5, 1e-4)
    np.testing.assert_allclose(nxt, nxt_o, rtol=rt, atol=at, err_msg=what + " next state")
    np.testing.assert_allclose(rew, P.ev.evaluate_next_reward(state, nxt, act), rtol=rr, atol=ra, err_msg=what + " reward")


def _case(L, monkeypatch, P, opt_name, path, mode, kernel=None, traced_only=False):
    """one case: `opt_name` on `path` (pendulum: a PENDULUM_TAILS path; learned: None, with the profile's kernel name)"""
    A, U, b = P.A, P.U, opt_name
    what = "%s %s/%s %s" % (P.name, opt_name, path or kernel, mode)
    if path is not None:                                 # the traced twin: the same arithmetic on the launch path that keeps a trace
        _set_path(monkeypatch, "fused" if path == "resident" else ("periter" if path == "fused-cma" else path))
    te = P.engine(L, opt_name)
    te.set_trace(True)
    r = B.Runner(opt_name, P.ev, P.lo, P.hi, A, mix=P.mix)
    reset, draws = B.case_draws(opt_name, A, U, B.case_seed(P.name, opt_name))
    if path is not None:
        _set_path(monkeypatch, path)
    pe = None if traced_only else P.engine(L, opt_name)
    engines = [e for e in (te, pe) if e is not None]
    if reset is not None:
        for e in engines:
            e.inject_noise(L.NOISE_PSO_RESET_POS, reset["uniform_pos"])
            e.inject_noise(L.NOISE_PSO_RESET_VEL, reset["uniform_vel"])
            e.reset()
        r.reset(reset)
        first = B.check_candidates(te.get_state("pos", (N, A, H, U)), r.opt.pos, P.lo, P.hi, 2e-5, what=what + " reset")
        assert np.all(first[2] >= 1)
        for e in engines:
            _check_state(P, e, r, _snapshot(r), what + " after reset()")
    cover = np.zeros((3, U), np.int64)
    noises, acts, snaps = [], [], []
    for t in range(STEPS):
        state = P.states[t]
        noise = draws[t] if mode == "injected" else _production(L, te, opt_name, t, A, U)
        if mode == "injected":
            _inject(L, te, opt_name, noise)
        noises.append(noise)
        out = te.optimize(state, t)
        act_o = r.step(state, noise, **_lock(L, P, te, r, state, what + " step %d" % t))
        rs_act = _check_trace(L, P, te, r, state, what + " step %d" % t, cover)
        acts.append(act_o if rs_act is None else rs_act)
        snaps.append(_snapshot(r))
        _check_step_outputs(P, b, out, acts[t], state, what + " traced step %d" % t)
        _check_state(P, te, r, snaps[t], what + " traced step %d" % t)
    if pe is not None:
        between = path != "resident"                     # any other entry point makes the resident kernel leave
        for t in range(STEPS):
            if mode == "injected":
                _inject(L, pe, opt_name, noises[t])
            out = pe.optimize(P.states[t], t)
            _check_step_outputs(P, b, out, acts[t], P.states[t], what + " step %d" % t)
            if between:
                _check_state(P, pe, r, snaps[t], what + " step %d" % t)
        _check_state(P, pe, r, snaps[-1], what + " last step")
        if path is not None:
            _assert_path(pe, _base(opt_name), path, A, STEPS)
        else:
            assert _kernel_ok(pe.get_profile()[2], kernel), (what, pe.get_profile()[2])
            assert _kernel_ok(te.get_profile()[2], kernel), (what, te.get_profile()[2])
    _close(*engines)
    return cover


# ---- a. the analytic pendulum: all six optimizers, every path ------------------------------------------------------
PENDULUM_PATHS = [(o2, p) for o, p in PENDULUM_TAILS for o2 in ((o, o + "-reset") if o == "PSO" else (o,))]


@pytest.mark.parametrize("bounds", list(B.PENDULUM_SETS))
@pytest.mark.parametrize("opt_name,path", PENDULUM_PATHS, ids=["%s-%s" % t for t in PENDULUM_PATHS])
def test_pendulum_optimizers_under_asymmetric_bounds(L, monkeypatch, opt_name, path, bounds):
    # the resident kernel takes no injection between its control steps (another entry point makes it leave): it runs on the
    # engine's own draws, which makes it the production-draw case (d) of RS / CEM / PI2 / SPSA as well
    mode = "production" if path == "resident" else "injected"
    cover = _case(L, monkeypatch, Problem(bounds, B.A), opt_name, path, mode)
    if opt_name in ("PI2", "CMA", "CMA-pa") and mode == "injected":      # (the same draws as tests/test_bounds_cpu.py, in lock-step)
        assert cover[0].sum() >= 1 and cover[1].sum() >= 1, cover


@pytest.mark.parametrize("opt_name,path", [("PSO", "periter"), ("PSO", "fused"), ("CMA", "periter"), ("CMA-pa", "periter"), ("CMA-pa", "fused-cma")])
def test_pendulum_production_draws_of_the_optimizers_without_a_resident_path(L, monkeypatch, opt_name, path):
    _case(L, monkeypatch, Problem("asym", B.A), opt_name, path, "production")


# ---- b. learned dynamics, U > 1 -----------------------------------------------------------------------------------
LEARNED_KERNEL = {"S20-U6-h200": "k_rollout_mlp_q4s", "S3-U2-h16": "k_rollout_mlp_w4"}


# (PSO-reset runs injected only: the draws of reset() are keyed apart from the control steps)
LEARNED = [(s_, o, m) for s_ in B.LEARNED_CASES for o in B.OPTIMIZERS for m in ("injected", "production") if (o, m) != ("PSO-reset", "production")]


@pytest.mark.parametrize("shape,opt_name,mode", LEARNED, ids=["%s-%s-%s" % t for t in LEARNED])
def test_learned_model_optimizers_under_per_dimension_bounds(L, monkeypatch, shape, opt_name, mode):
    cover = _case(L, monkeypatch, Problem(shape, B.A), opt_name, None, mode, kernel=LEARNED_KERNEL[shape])
    if opt_name in ("PI2", "CMA", "CMA-pa") and mode == "injected":
        assert np.all(cover[0] >= 1) and np.all(cover[1] >= 1), cover     # every action dimension clips on both sides


# ---- c. every other kernel that forms candidates from the bounds: the uniform map (RS), the sigma constraint + refit (CEM),
# ---- clip + penalty (PI2) ------------------------------------------------------------------------------------------------
KERNELS = [(v, o) for v in VARIANTS for o in ("RS", "CEM", "PI2") if not (v == "corr" and o == "RS")]      # (RS draws are not mixed)


@pytest.mark.parametrize("variant,opt_name", KERNELS, ids=["%s-%s" % t for t in KERNELS])
def test_other_candidate_forming_kernels_under_per_dimension_bounds(L, monkeypatch, variant, opt_name):
    name, env, kernel = VARIANTS[variant]
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    P = Problem(name, B.A, variant)
    cover = _case(L, monkeypatch, P, opt_name, None, "injected", kernel=kernel)
    if variant == "corr":
        probe = P.engine(L, opt_name)
        assert probe.sampling_correlation_installed()
        _close(probe)
    if opt_name == "PI2" or (variant == "corr" and opt_name == "CEM"):
        assert np.all(cover[0] + cover[1] >= 1), cover      # every dimension clips (both sides, PI2: tests/test_bounds_cpu.py)


# ---- e. agent sharding ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opt_name", ["CEM", "PSO"])
def test_agent_shards_equal_the_unsharded_engine_bit_for_bit(L, opt_name):
    # a bound indexed through a local, agent-dependent offset would differ between a shard and the full engine
    A = 4
    P = Problem("S20-U6-h200", A)
    full = P.engine(L, opt_name)
    outs = [full.optimize(P.states[t], t) for t in range(STEPS)]
    prev = full.get_state("prev_mean") if opt_name == "CEM" else full.get_state("pos", (N, A, H, P.U))
    for off in (0, 2):
        sh = Problem("S20-U6-h200", 2).engine(L, opt_name, agent_offset=off, num_agents_global=A)
        for t in range(STEPS):
            got = sh.optimize(P.states[t][off:off + 2], t)
            for g, f in zip(got, outs[t]):
                np.testing.assert_array_equal(g, f[off:off + 2], err_msg="agent_offset %d step %d" % (off, t))
        if opt_name == "CEM":
            np.testing.assert_array_equal(sh.get_state("prev_mean"), prev[off:off + 2])
        else:
            np.testing.assert_array_equal(sh.get_state("pos", (N, 2, H, P.U)), prev[:, off:off + 2])
        _close(sh)
    _close(full)
