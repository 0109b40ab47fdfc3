"""Trajectory distributions on the GPU (include/bbmpc.h: bbmpc_predict_trajectory_particles): zero noise against the
deterministic prediction, the particle tensors against the NumPy statements of tests/traj_particles_util.py with supplied
noise (plain, ensemble and Gaussian kinds, the pendulum), consistency with bbmpc_evaluate_particles, the handle's own
draws, the moments, refusals and lifecycle, and the Python classes.

Shapes: B in {5, 9}, P = 4, E in {1, 2}, Hq in {1, 7} on handles whose planning horizon is 3 -- B * P / E = 10 is one partial
16-row tile, 18 a full and a partial one, 20 and 36 several; NARROW (16 hidden units: one wave, 16 S = 320 > 2 * 64) and
mlp32 (two waves, 320 > 256) fetch noise past the registers, SWISH / mlp200_swish are EXT kernels."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import particle_util as PU
from tests import traj_particles_util as TP
from tests import traj_util as T
from tests.test_gaussian_cpu import gaussian_case
from tests.test_particles_cpu import PEND_SIGMA

pytestmark = pytest.mark.gpu

F = np.float32
P4 = 4
H_HANDLE = 3
SHAPES = [(5, 1), (5, 7), (9, 7)]                     # (B, Hq)
PENDULUM_EV = O.Evaluator("pendulum", O.Handler(O.pendulum_dynamics, True))
# gaussian_case indices used below: 3 (CHEETAH, E 2), 5 (PEND_MLP raw, E 2), 6 (NARROW, E 1), 7 (NARROW, E 2), all P 4; 4 (SWISH, P 6, E 3)


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device visible"
    return _lib


def _pendulum_engine(L, A=2, H=H_HANDLE, strict=False, **kw):
    from blackbox_mpc_amd.engine import Engine
    return Engine(kw.pop("opt", L.OPT_NONE), L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=A, planning_horizon=H,
                  quirks=L.STRICT_MATH if strict else 0, **kw)


def _pendulum_rows(B, Hq, P=P4, seed=0):
    rng = np.random.default_rng(B * 100 + Hq + seed)
    return (np.ascontiguousarray(O.pendulum_start_states(B), F), rng.uniform(-2, 2, (B, Hq, 1)).astype(F),
            rng.standard_normal((B, P, Hq, 3)).astype(F))


def _mlp_engine(L, c, A=2, H=H_HANDLE, reward=None):
    from tests.test_gpu_predict_trajectories import _mlp_engine as make
    return make(L, c, horizon=H, agents=A, reward=reward)


def _member_engine(L, c, A=2, H=H_HANDLE, heads=True, ensemble=True, **kw):
    """The handle of tests/test_gpu_gaussian.py for gaussian_case `c`: member 0 as the model, then members and heads."""
    from tests.test_gpu_gaussian import _engine
    eng = _engine(L, c["spec"], c["params"], c["stats"], A, H, **kw)
    if ensemble and len(c["params"]) > 1:
        eng.set_mlp_ensemble(c["params"])
    if heads:
        eng.set_mlp_logvar_head(c["raw_heads"], *c["bounds"])
    return eng


def _member_rows(c, B, Hq, P, seed):
    S, U, reward = c["spec"][2], c["spec"][3], c["spec"][4]
    rng = np.random.default_rng(seed)
    states = (O.cheetah_start_states(B, S) if reward == "cheetah" else O.pendulum_start_states(B)).astype(F)
    return states, rng.uniform(-1, 1, (B, Hq, U)).astype(F), rng.standard_normal((B, P, Hq, S)).astype(F)


# ---- 1. zero noise is the deterministic prediction -----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mlp200_raw_B77_H30", "mlp32_norm_B1_H50", "mlp200_swish_B77_H30", "mlp64_S17U6_B77_H30"])
@pytest.mark.parametrize("P,E", [(1, 1), (4, 1), (4, 2)])
def test_zero_sigma_is_predict_trajectories_bit_for_bit_mlp(L, name, P, E):
    c = T.mlp_case(name)
    eng = _mlp_engine(L, c)
    for B, Hq in SHAPES:
        states, seq = TP.rows_for(c, B, Hq, 7 * B + Hq)
        want_s, want_r = eng.predict_trajectories(states, seq)
        eng.set_particles(P, np.zeros(c["S"], F), 0.0)
        if E > 1:
            eng.set_mlp_ensemble([(c["ws"], c["bs"])] * E)                # E copies of the primary
        eps = np.random.default_rng(B).standard_normal((B, P, Hq, c["S"])).astype(F)      # (multiplied by sigma = 0)
        sm, ss, rm, rs, ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
        for p in range(P):
            np.testing.assert_array_equal(ps[:, p], want_s)
            np.testing.assert_array_equal(pr[:, p], want_r)
        np.testing.assert_array_equal(sm, want_s)
        np.testing.assert_array_equal(rm, want_r)
        assert np.all(ss == 0) and np.all(rs == 0)
        eng.set_mlp_ensemble([])
        eng.set_particles(0)


@pytest.mark.parametrize("P", [1, 4])
def test_zero_sigma_is_the_strict_pendulum_prediction_bit_for_bit(L, P):
    eng, det = _pendulum_engine(L), _pendulum_engine(L, strict=True)
    eng.set_particles(P, np.zeros(3, F), 0.0)
    for B, Hq in SHAPES + [(77, 7)]:                                       # (77 * 4 rows: several waves)
        states, seq, eps = _pendulum_rows(B, Hq, P)
        want_s, want_r = det.predict_trajectories(states, seq)
        sm, ss, rm, rs, ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
        for p in range(P):
            np.testing.assert_array_equal(ps[:, p], want_s)
            np.testing.assert_array_equal(pr[:, p], want_r)
        np.testing.assert_array_equal(sm, want_s)
        np.testing.assert_array_equal(rm, want_r)
        assert np.all(ss == 0) and np.all(rs == 0)


# ---- 2. against the oracles, eps supplied --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Hq", SHAPES)
def test_pendulum_particles_against_the_oracle(L, B, Hq):
    states, seq, eps = _pendulum_rows(B, Hq)
    eng = _pendulum_engine(L)
    eng.set_particles(P4, PEND_SIGMA, 0.0)
    ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)[4:]
    o_s, o_r = TP.oracle_particles([PENDULUM_EV], None, states, seq, eps, PEND_SIGMA)
    r_s, r_r = TP.particles64(T.pendulum_step64, states, seq, eps, PEND_SIGMA)
    what = "pendulum B=%d Hq=%d" % (B, Hq)
    T.check_against_float64(TP.steps_first(ps), TP.steps_first(o_s), TP.steps_first(r_s), T.STATE_RTOL, T.STATE_ATOL, what + " states")
    T.check_against_float64(TP.steps_first(pr), TP.steps_first(o_r), TP.steps_first(r_r), T.REWARD_RTOL, T.REWARD_ATOL, what + " rewards")
    TP.check_lockstep([PENDULUM_EV], None, states, seq, eps, PEND_SIGMA, ps, pr, what)
    assert np.all(np.ptp(ps, axis=1) > 0)                                  # (the particles do differ)


@pytest.mark.parametrize("name", ["mlp200_raw_B77_H30", "mlp32_norm_B1_H50", "mlp64_S17U6_B77_H30"])
@pytest.mark.parametrize("B,Hq", SHAPES)
def test_plain_mlp_particles_against_the_oracle(L, name, B, Hq):
    c = T.mlp_case(name)
    states, seq = TP.rows_for(c, B, Hq, 11 * B + Hq)
    eps = np.random.default_rng(B + Hq).standard_normal((B, P4, Hq, c["S"])).astype(F)
    sigma = np.full(c["S"], 0.02, F)
    eng = _mlp_engine(L, c)
    eng.set_particles(P4, sigma, 0.0)
    ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)[4:]
    ev = T.oracle_mlp_evaluator(c)
    o_s, o_r = TP.oracle_particles([ev], None, states, seq, eps, sigma)
    r_s, r_r = TP.particles64(T.Mlp64(c["ws"], c["bs"], c["acts"], c["stats"]), states, seq, eps, sigma)
    what = "%s B=%d Hq=%d" % (name, B, Hq)
    T.check_against_float64(TP.steps_first(ps), TP.steps_first(o_s), TP.steps_first(r_s), T.STATE_RTOL, T.STATE_ATOL, what + " states")
    T.check_against_float64(TP.steps_first(pr), TP.steps_first(o_r), TP.steps_first(r_r), T.REWARD_RTOL, T.REWARD_ATOL, what + " rewards")
    TP.check_lockstep([ev], None, states, seq, eps, sigma, ps, pr, what)


@pytest.mark.parametrize("heads", [False, True])
@pytest.mark.parametrize("case,P", [(3, 4), (5, 4), (6, 4), (7, 4), (4, 6)])
@pytest.mark.parametrize("B,Hq", SHAPES)
def test_ensemble_and_gaussian_particles_in_lock_step_with_the_oracle(L, case, P, heads, B, Hq):
    """no float64 restatement of the members / heads exists: every step from the device's own previous state"""
    c = gaussian_case(case)
    E = len(c["params"])
    states, seq, eps = _member_rows(c, B, Hq, P, 100 * case + 10 * B + Hq)
    eng = _member_engine(L, c, heads=heads)
    eng.set_particles(P, c["sigma"], 0.0)
    ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)[4:]
    TP.check_lockstep(c["evs"], c["heads"] if heads else None, states, seq, eps, c["sigma"], ps, pr,
                      "case %d E=%d heads=%s B=%d Hq=%d" % (case, E, heads, B, Hq))
    if E > 1 and Hq > 1:                                                   # member p % E: particles 0 and 1 follow different networks
        quiet = eng.predict_trajectory_particles(states, seq, eps=np.zeros_like(eps), want_particles=True)[4]
        assert not np.array_equal(quiet[:, 0], quiet[:, 1])
        if not heads:
            np.testing.assert_array_equal(quiet[:, 0], quiet[:, E])


# ---- 3. consistent with evaluate_particles -------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "gauss"])
def test_step_rewards_sum_to_the_returns_of_evaluate_particles(L, kind):
    A, H = 5, 7
    if kind == "pendulum":
        eng = _pendulum_engine(L, A=A, H=H, seed=21)
        states, seq, eps = _pendulum_rows(A, H)
        eng.set_particles(P4, PEND_SIGMA, 0.0)
    else:
        c = gaussian_case(5)
        eng = _member_engine(L, c, A=A, H=H, seed=21)
        states, seq, eps = _member_rows(c, A, H, P4, 5)
        eng.set_particles(P4, c["sigma"], 0.0)
    for own in (False, True):
        eng.inject_noise(L.NOISE_PROCESS, None if own else eps)            # [A,P,H,S]: here B = A, Hq = H
        returns = eng.evaluate_particles(states, seq[None])[1]             # [1, P, A]
        pr = eng.predict_trajectory_particles(states, seq, eps=None if own else eps, want_particles=True)[5]
        got = pr.sum(-1, dtype=F)                                          # [A, P]
        print("[%s own=%s] max |sum_t r - return| = %.3e" % (kind, own, np.abs(got - returns[0].T).max()))
        np.testing.assert_allclose(got, returns[0].T, rtol=1e-3, atol=1e-3 * H)
        assert np.all(np.ptp(got, axis=1) > 0)


# ---- 4. the handle's own draws -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "mlp"])
def test_own_draws_are_the_documented_process_noise(L, kind):
    """eps = NULL is a call with the generator's tensor for (seed, current control step, iteration 0, B rows in the agent
    word, Qp of Hq * S): bit for bit against the tensor the device generator itself gives for that key (dumped from a
    handle of num_agents = B, planning_horizon = Hq), which in turn is particle_util.process_noise_np to the float32
    Box-Muller tolerance of tests/test_gpu_particles.py (2e-5) -- a float64 host evaluation cannot give the device's bits.
    With the host tensor passed as eps the trajectories agree to the one-step tolerance (noise deviations of 2e-5 sigma)."""
    seed, off, B, Hq = 0x1234567890ABCDEF, 3, 9, 7
    if kind == "pendulum":
        eng = _pendulum_engine(L, seed=seed, agent_offset=off, num_agents_global=8)
        twin = _pendulum_engine(L, A=B, H=Hq, seed=seed, agent_offset=off, num_agents_global=B + off)
        states, seq, _ = _pendulum_rows(B, Hq)
        sigma, S = PEND_SIGMA, 3
    else:
        c = T.mlp_case("mlp64_S17U6_B77_H30")                              # Hq * S = 119: a ragged last Philox block
        from blackbox_mpc_amd.engine import Engine
        from tests.test_gpu_predict_trajectories import CODE

        def make(A, H):
            e = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-1.0] * c["U"], [1.0] * c["U"], dim_s=c["S"], num_agents=A,
                       planning_horizon=H, seed=seed, agent_offset=off, num_agents_global=A + off)
            e.set_mlp(c["ws"], c["bs"], [CODE[a] for a in c["acts"]], c["stats"])
            return e
        eng, twin = make(2, H_HANDLE), make(B, Hq)
        states, seq = TP.rows_for(c, B, Hq, 1)
        sigma, S = np.full(c["S"], 0.02, F), c["S"]
    eng.set_particles(P4, sigma, 0.0)
    twin.set_particles(P4, sigma, 0.0)
    own = eng.predict_trajectory_particles(states, seq, want_particles=True)
    again = eng.predict_trajectory_particles(states, seq, want_particles=True)
    for a, b in zip(own, again):
        np.testing.assert_array_equal(a, b)                                # equal calls, equal bits
    dumped = twin.dump_noise(L.NOISE_PROCESS, 0, 0, (B, P4, Hq, S))
    host = PU.process_noise_np(seed, 0, 0, B, P4, Hq, S, agent_offset=off)
    np.testing.assert_allclose(dumped, host, rtol=0, atol=2e-5)
    fed = eng.predict_trajectory_particles(states, seq, eps=dumped, want_particles=True)
    for a, b in zip(own, fed):
        np.testing.assert_array_equal(a, b)
    fed_host = eng.predict_trajectory_particles(states, seq, eps=host.astype(F), want_particles=True)
    np.testing.assert_allclose(own[4], fed_host[4], rtol=T.STATE_RTOL, atol=T.STATE_ATOL)
    assert np.all(np.ptp(own[4], axis=1) > 0)
    # the dedicated buffer: a call in between leaves the draws of the control step's own process noise alone
    before = eng.evaluate_particles(states[:2], np.zeros((3, 2, H_HANDLE, seq.shape[2]), F))[1]
    eng.predict_trajectory_particles(states, seq)
    np.testing.assert_array_equal(eng.evaluate_particles(states[:2], np.zeros((3, 2, H_HANDLE, seq.shape[2]), F))[1], before)


# ---- 5. moments ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["pendulum", "gauss"])
def test_moments_are_the_float32_restatement_of_the_particle_tensors(L, kind):
    B, Hq = 9, 7
    if kind == "pendulum":
        eng = _pendulum_engine(L)
        states, seq, eps = _pendulum_rows(B, Hq)
        sigma = np.array([0.05, 0.05, 0.25], F)
    else:
        c = gaussian_case(6)                                               # (one model with a head: P = 1 below is allowed)
        eng = _member_engine(L, c)
        states, seq, eps = _member_rows(c, B, Hq, P4, 9)
        sigma = c["sigma"]
    eng.set_particles(P4, sigma, 0.0)
    sm, ss, rm, rs, ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
    TP.check_moments(sm, ss, ps, kind + " states")
    TP.check_moments(rm, rs, pr, kind + " rewards")
    # without the particle outputs (the rollout writes to the handle's scratch): the same moments
    for a, b in zip(eng.predict_trajectory_particles(states, seq, eps=eps), (sm, ss, rm, rs)):
        np.testing.assert_array_equal(a, b)
    # any subset of the outputs may be null
    full = (sm, ss, rm, rs, ps, pr)
    for mask in (0b000001, 0b000010, 0b000100, 0b001000, 0b010000, 0b100000, 0b001010, 0b110101):
        outs = [np.full_like(full[i], np.nan) if mask >> i & 1 else None for i in range(6)]
        L.check(L.lib.bbmpc_predict_trajectory_particles(eng._h, L.ptr(L.f32c(states)), L.ptr(L.f32c(seq)), B, Hq, L.ptr(eps),
                                                         *[L.ptr(o) for o in outs]))
        for o, w in zip(outs, full):
            if o is not None:
                np.testing.assert_array_equal(o, w)
    # P = 1: the mean is the particle, the std exactly 0
    eng.set_particles(1, sigma, 0.0)
    sm, ss, rm, rs, ps, pr = eng.predict_trajectory_particles(states, seq, eps=eps[:, :1], want_particles=True)
    np.testing.assert_array_equal(sm, ps[:, 0])
    np.testing.assert_array_equal(rm, pr[:, 0])
    assert np.all(ss == 0) and np.all(rs == 0)
    # the _dev form on torch tensors gives the host form's bits
    import torch
    eng.set_particles(P4, sigma, 0.0)
    dev = torch.device("cuda", eng.device)
    d_s, d_q, d_e = (torch.from_numpy(np.ascontiguousarray(v, F)).to(dev) for v in (states, seq, eps))
    d_sm, d_ss = torch.empty((B, Hq, eng.S), device=dev), torch.empty((B, Hq, eng.S), device=dev)
    torch.cuda.synchronize(dev)
    eng.predict_trajectory_particles_dev(d_s.data_ptr(), d_q.data_ptr(), B, Hq, d_e.data_ptr(), d_sm.data_ptr(), d_ss.data_ptr())
    eng.synchronize()
    np.testing.assert_array_equal(d_sm.cpu().numpy(), full[0])
    np.testing.assert_array_equal(d_ss.cpu().numpy(), full[1])


# ---- 6. refusals and lifecycle ---------------------------------------------------------------------------------------------
def test_refusals(L):
    eng = _pendulum_engine(L)
    states, seq, eps = _pendulum_rows(5, 7)
    buf = np.zeros(5 * 4 * 7 * 3, F)

    def call(e, batch, hq, outs=(1, 0, 0, 0, 0, 0)):
        return L.lib.bbmpc_predict_trajectory_particles(e._h, L.ptr(states), L.ptr(seq), batch, hq, None,
                                                        *[L.ptr(buf) if o else None for o in outs])
    assert call(eng, 5, 7) == L.E_STATE and b"bbmpc_set_particles" in L.lib.bbmpc_last_error()
    with pytest.raises(ValueError, match="set_particles"):
        eng.predict_trajectory_particles(states, seq)
    eng.set_particles(P4, PEND_SIGMA, 0.0)
    assert call(eng, 5, 7) == 0
    assert call(eng, 0, 7) == L.E_INVALID and call(eng, -1, 7) == L.E_INVALID
    assert call(eng, 5, 0) == L.E_INVALID and call(eng, 5, 4097) == L.E_INVALID
    assert call(eng, 5, 7, (0,) * 6) == L.E_INVALID
    assert L.lib.bbmpc_predict_trajectory_particles(eng._h, None, L.ptr(seq), 5, 7, None, L.ptr(buf), None, None, None, None, None) == L.E_INVALID
    # sizes are refused before anything is allocated or read: B * P * Hq * S >= 2^31
    assert call(eng, 2 ** 31 // (4 * 4096 * 3) + 1, 4096) == L.E_UNSUPPORTED
    assert L.lib.bbmpc_predict_trajectory_particles_dev(eng._h, 1, 1, 2 ** 31 // (4 * 4096 * 3) + 1, 4096, None, 1, None, None, None, None,
                                                        None) == L.E_UNSUPPORTED
    eng.set_particles(0)
    assert call(eng, 5, 7) == L.E_STATE
    # a learned model without weights
    from blackbox_mpc_amd.engine import Engine
    bare = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-1.0], [1.0], dim_s=3, num_agents=1, planning_horizon=3)
    bare.set_particles(P4, PEND_SIGMA, 0.0)
    assert call(bare, 5, 7) == L.E_STATE and b"bbmpc_set_mlp" in L.lib.bbmpc_last_error()


def test_serves_a_handle_with_an_optimizer_and_a_resident_kernel_and_leaves_the_control_step_alone(L):
    from blackbox_mpc_amd.engine import Engine

    def make():
        return Engine(L.OPT_CEM, L.DYN_PENDULUM, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=10,
                      population_size=128, max_iterations=2, num_elite=16, seed=1)
    eng, ref = make(), make()
    st = O.pendulum_start_states(1)
    states, seq, eps = _pendulum_rows(9, 7)
    a0, r0 = eng.optimize(st), ref.optimize(st)                            # (the control-step kernel may stay resident)
    for x, y in zip(a0, r0):
        np.testing.assert_array_equal(x, y)
    eng.set_particles(P4, PEND_SIGMA, 0.0)
    got = eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)
    fresh = _pendulum_engine(L)
    fresh.set_particles(P4, PEND_SIGMA, 0.0)
    for x, y in zip(got, fresh.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)):
        np.testing.assert_array_equal(x, y)
    # own draws are keyed by the handle's current control step: one step taken, so step 1
    own = eng.predict_trajectory_particles(states, seq, want_particles=True)
    twin = _pendulum_engine(L, A=9, H=7, seed=1)
    twin.set_particles(P4, PEND_SIGMA, 0.0)
    fed = fresh.predict_trajectory_particles(states, seq, eps=twin.dump_noise(L.NOISE_PROCESS, 1, 0, (9, P4, 7, 3)), want_particles=True)
    for x, y in zip(own, fed):
        np.testing.assert_array_equal(x, y)
    # num_particles = 0 afterwards: the deterministic control step's bits
    eng.set_particles(0)
    for t in range(3):
        for x, y in zip(eng.optimize(st), ref.optimize(st)):
            np.testing.assert_array_equal(x, y)


# ---- 7. Python -------------------------------------------------------------------------------------------------------------
def _handler(kind):
    from blackbox_mpc_amd.dynamics_functions import EnsembleMLP, ProbabilisticMLP
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    from blackbox_mpc_amd.spaces import Box
    from tests.test_gpu_mlp import _stats
    act_space, obs_space = Box([-2.0], [2.0]), Box([-1, -1, -8], [1, 1, 8])
    layers, acts = [4, 32, 32, 3], ["tanh", "tanh", None]
    if kind == "ensemble":
        fn = EnsembleMLP(layers, acts, num_members=2, seed=9)
        models = fn.members
    elif kind == "probabilistic":
        fn = ProbabilisticMLP(layers, acts, min_logvar=-8.0, max_logvar=-2.0, seed=9)
        models = [fn]
    else:
        fn = DeterministicMLP(layers, acts)
        rng = np.random.default_rng(9)
        fn.set_weights([rng.normal(0, 0.3, w.shape).astype(F) for w in fn.weights], [rng.normal(0, 0.05, b.shape).astype(F) for b in fn.biases])
        models = [fn]
    for m in models:                                                       # small outputs: the pendulum's range
        m.set_weights(m.weights[:-1] + [m.weights[-1] * F(0.1)], m.biases)
    handler = SystemDynamicsHandler(act_space, obs_space, dynamics_function=fn, is_normalized=True)
    stats = _stats(3, 1, 44)
    handler.set_normalization_stats(*stats)
    return handler, fn, models, stats, act_space, obs_space


@pytest.mark.parametrize("kind", ["deterministic", "ensemble", "probabilistic"])
def test_predict_trajectory_distribution_and_calibration(L, kind):
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import calibration_z_rms, multistep_windows
    from blackbox_mpc_amd.engine import Engine
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    handler, fn, models, stats, _, _ = _handler(kind)
    sigma = np.array([0.01, 0.01, 0.05], F)
    ev = ParticleTrajectoryEvaluator(pendulum_reward_function, handler, num_particles=P4, process_noise_std=sigma)
    states, seq, eps = _pendulum_rows(9, 7)
    out = ev.predict_trajectory_distribution(states, seq, eps=eps, return_particles=True)
    assert [o.shape for o in out] == [(9, 7, 3), (9, 7, 3), (9, 7), (9, 7), (9, P4, 7, 3), (9, P4, 7)]
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=1)
    eng.set_mlp(fn.weights, fn.biases, fn.activation_codes, stats)
    if kind == "ensemble":
        eng.set_mlp_ensemble(models)
    if kind == "probabilistic":
        eng.set_mlp_logvar_head(models, fn.min_logvar, fn.max_logvar)
    eng.set_particles(P4, sigma, 0.0)
    for a, b in zip(out, eng.predict_trajectory_particles(states, seq, eps=eps, want_particles=True)):
        np.testing.assert_array_equal(a, b)
    assert len(ev.predict_trajectory_distribution(states, seq)) == 4 and np.all(out[1] > 0)
    # the calibration is calibration_z_rms of the evaluator's own output on the windows
    rng = np.random.default_rng(2)
    obs_all = [rng.standard_normal((12, 2, 3)).astype(F) * F(0.3), rng.standard_normal((4, 2, 3)).astype(F) * F(0.3)]
    act_all = [rng.uniform(-2, 2, (11, 2, 1)).astype(F), rng.uniform(-2, 2, (3, 2, 1)).astype(F)]
    z, n = handler.multistep_calibration(obs_all, act_all, 5, 2, ev)
    starts, acts, observed = multistep_windows(obs_all, act_all, 5, 2)
    assert n == starts.shape[0] == 8 and z.shape == (5, 3)
    mean, std = ev.predict_trajectory_distribution(starts, acts)[:2]
    np.testing.assert_array_equal(z, calibration_z_rms(mean, std, observed))
    assert np.all(np.isfinite(z)) and handler.multistep_z_rms[1] == n


@pytest.mark.parametrize("model", ["pendulum", "mlp"])
def test_plan_distribution(L, model):
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from tests.test_gpu_predict_trajectories import OPTIMIZERS, PLAN_A, PLAN_H, _plan_policy
    det, start = _plan_policy(model, "CEM")
    with pytest.raises(TypeError, match="ParticleTrajectoryEvaluator"):
        det.plan_distribution(start)                                       # a deterministic evaluator has no distribution
    base = det._trajectory_evaluator
    S = base._system_dynamics_handler._dim_S

    def policy(sigma):
        ev = ParticleTrajectoryEvaluator(base._reward_function, base._system_dynamics_handler, num_particles=P4, process_noise_std=sigma)
        return MPCPolicy(trajectory_evaluator=ev, env_action_space=det._optimizer._env_action_space,
                         env_observation_space=det._optimizer._env_observation_space, optimizer_name="CEM", num_agents=PLAN_A,
                         planning_horizon=PLAN_H, seed=3, **OPTIMIZERS["CEM"])
    pol = policy(np.zeros(S, F))
    pol.act(start, 0)
    with pytest.raises(RuntimeError, match="keep_plan"):
        pol.plan_distribution(start)
    pol.keep_plan(True)
    action, nxt, rew = pol.act(start, 1)
    acts, sm, ss, rm, rs = pol.plan_distribution(start)
    eng = pol._optimizer._engine
    assert acts.shape == (PLAN_A, PLAN_H, eng.U) and sm.shape == ss.shape == (PLAN_A, PLAN_H, S) and rm.shape == rs.shape == (PLAN_A, PLAN_H)
    assert np.array_equal(acts[:, 0], action) and np.array_equal(acts, pol.plan(start)[0])
    np.testing.assert_allclose(sm[:, 0], nxt, rtol=2e-5, atol=2e-5)        # sigma = 0: the record's predicted next state
    assert np.all(ss == 0) and np.all(rs == 0)
    one = pol.plan_distribution(start[0])                                  # 1-D un-batching, as plan
    assert one[0].shape == (PLAN_H, eng.U) and np.array_equal(one[1], sm[0]) and len(one) == 5
    noisy = policy(np.full(S, 0.05, F))
    noisy.keep_plan(True)
    noisy.act(start, 0)
    out = noisy.plan_distribution(start)
    assert np.all(out[2] > 0) and np.all(out[4][:, 1:] > 0) and np.all(np.isfinite(out[1]))
