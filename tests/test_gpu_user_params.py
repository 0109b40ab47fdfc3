"""Runtime parameters of HIP-source reward / dynamics functions (bbmpc_set_*_source_params, bbmpc_set_user_params).

A parameterised function sees its agent's parameter row and the planning step t in every kernel that calls it.  Checked:
 * equivalence to the same function with the parameters written as literals, on every kernel path: the fused analytic
   rollout (built-in and user partners), the step-wise evaluator, the learned model's trajectory scorers (w4, q4s and
   the pipelined pair kernel) and its transform rollout -- rtol 1e-5;
 * per-agent goals and per-agent masses against a NumPy restatement, one agent at a time (pendulum tolerances);
 * t reaches the function: a reward that tracks a reference trajectory params[t * S + i];
 * live updates between MPCPolicy.act calls move the goal without a recompile, in step with a torch-callable reward
   that closes over a CUDA goal tensor (same seed, same draws);
 * the record's reward at t = 0 uses each agent's own row (act, rollout_on_device);
 * agent shards upload their own rows of one [num_agents_global, P] parameter set;
 * refusals: a wrong count, a one-step call whose rows are not a multiple of the agents, computing before setting.
Every test runs on both user-rollout forms (the default and BBMPC_USER_STEPWISE=1)."""
import threading

import numpy as np
import pytest

from oracle import oracle_np as O

pytestmark = pytest.mark.gpu
F = np.float32
LO, HI = [-2.0], [2.0]
R_RTOL, R_ATOL = 2e-4, 2e-3                                  # the suite's pendulum tolerances

from tests.test_gpu_user_functions import USER_PENDULUM_MODEL      # noqa: E402

REWARD_SIG = ("bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U)",
              "bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U, "
              "const float* params, int t)")
DYNAMICS_SIG = ("bbmpc_user_dynamics(const float* x, float* delta, int S, int U)",
                "bbmpc_user_dynamics_params(const float* x, float* delta, int S, int U, const float* params, int t)")

# $k: params[k] in the parameterised form, a literal in the classic one
GOAL_REWARD = """
__device__ float @SIG@ {
    const float d0 = nxt[0] - $0, d1 = nxt[S - 1] - $1;
    float ss = 0.0f;
    for (int u = 0; u < U; ++u) ss = ss + act[u] * act[u];
    return (-(d0 * d0) - d1 * d1) - $2 * ss;
}
"""
# the pendulum's angle against a target angle
ANGLE_REWARD = """
__device__ float @SIG@ {
    const float th = atan2f(nxt[1], nxt[0]);
    const float d = th - $0;
    return -(d * d) - $1 * (act[0] * act[0]);
}
"""
# tests/test_gpu_user_functions.py's user pendulum with the torque divided by a mass
MASS_PENDULUM = """
__device__ void @SIG@ {
    const float PI = 3.14159274101257324f;
    const float th = atan2f(x[1], x[0]);
    float acc = -15.0f * sinf(th + PI);
    acc = acc + (3.0f / $0) * x[3];
    float nthd = x[2] + acc * 0.05f;
    const float nth = th + nthd * 0.05f;
    nthd = fminf(fmaxf(nthd, -8.0f), 8.0f);
    delta[0] = cosf(nth) - x[0];
    delta[1] = sinf(nth) - x[1];
    delta[2] = nthd - x[2];
}
"""
# a reference trajectory: params[t * S + i] is the state wanted after step t
TRACKING_REWARD = """
__device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
                                          const float* params, int t) {
    float r = 0.0f;
    for (int i = 0; i < S; ++i) {
        const float d = nxt[i] - params[t * S + i];
        r = r - d * d;
    }
    return r;
}
"""
IDENTITY_XFORM = """
__device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S) {
    for (int i = 0; i < S; ++i) next[i] = cur[i] + 0.5f * dev[i];
}
"""


def _forms(template, sig, values):
    """(parameterised source, classic source with `values` as literals)"""
    par, lit = template.replace("@SIG@", sig[1]), template.replace("@SIG@", sig[0])
    for k, v in enumerate(values):
        par = par.replace("$%d" % k, "params[%d]" % k)
        lit = lit.replace("$%d" % k, "%sf" % repr(float(v)))
    return par, lit


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(params=["fused", "stepwise"], autouse=True)
def user_rollout_form(request, monkeypatch):
    if request.param == "stepwise":
        monkeypatch.setenv("BBMPC_USER_STEPWISE", "1")
    yield request.param


def _engine(L, dyn, rew, A, H, S=3, lo=LO, hi=HI):
    from blackbox_mpc_amd.engine import Engine
    return Engine(L.OPT_NONE, dyn, rew, lo, hi, dim_s=S, num_agents=A, planning_horizon=H)


def _np_angle_reward(goal, w):
    def r(cur, act, nxt):
        th = np.arctan2(nxt[:, 1], nxt[:, 0]).astype(F)
        d = (th - F(goal)).astype(F)
        return (-(d * d) - F(w) * (act[:, 0] * act[:, 0])).astype(F)
    return r


def _np_mass_pendulum(m):
    def f(x):
        x = x.astype(F)
        PI = F(3.14159274101257324)
        th = np.arctan2(x[:, 1], x[:, 0]).astype(F)
        acc = (F(-15.0) * np.sin(th + PI)).astype(F)
        acc = (acc + (F(3.0) / F(m)) * x[:, 3]).astype(F)
        nthd = (x[:, 2] + acc * F(0.05)).astype(F)
        nth = (th + nthd * F(0.05)).astype(F)
        nthd = np.clip(nthd, F(-8.0), F(8.0))
        return np.stack([np.cos(nth) - x[:, 0], np.sin(nth) - x[:, 1], nthd - x[:, 2]], axis=1).astype(F)
    return f


# ---- 1. equivalence to literals ---------------------------------------------------------------------------------------
def test_analytic_paths_match_the_literal_source(L):
    A, H, N = 2, 12, 200
    goal = [0.75, -0.5, 0.125]
    rp, rl = _forms(GOAL_REWARD, REWARD_SIG, goal)
    dp, dl = _forms(MASS_PENDULUM, DYNAMICS_SIG, [2.0])
    rng = np.random.default_rng(3)
    states = O.pendulum_start_states(A)
    seq = rng.uniform(-2, 2, (N, A, H, 1)).astype(F)
    # user reward + user dynamics, both parameterised (shared rows) / both literal
    par, lit = _engine(L, L.DYN_USER, L.REW_USER, A, H), _engine(L, L.DYN_USER, L.REW_USER, A, H)
    par.set_reward_source(rp, 3)
    par.set_dynamics_source(dp, 1)
    par.set_user_params(L.USER_KIND_REWARD, goal)
    par.set_user_params(L.USER_KIND_DYNAMICS, [2.0])
    lit.set_reward_source(rl)
    lit.set_dynamics_source(dl)
    np.testing.assert_allclose(par.evaluate(states, seq), lit.evaluate(states, seq), rtol=1e-5, atol=1e-5)
    s, a = states, seq[0, :, 0]
    np.testing.assert_allclose(par.predict_next_state(s, a), lit.predict_next_state(s, a), rtol=1e-5, atol=1e-6)
    n = lit.predict_next_state(s, a)
    np.testing.assert_allclose(par.evaluate_next_reward(s, n, a), lit.evaluate_next_reward(s, n, a), rtol=1e-5, atol=1e-6)
    # each with a built-in partner: the parameterised reward on the built-in pendulum model, the parameterised model
    # under the built-in pendulum reward
    for dyn, rew in ((L.DYN_PENDULUM, L.REW_USER), (L.DYN_USER, L.REW_PENDULUM)):
        par, lit = _engine(L, dyn, rew, A, H), _engine(L, dyn, rew, A, H)
        if rew == L.REW_USER:
            par.set_reward_source(rp, 3)
            par.set_user_params(L.USER_KIND_REWARD, goal)
            lit.set_reward_source(rl)
        else:
            par.set_dynamics_source(dp, 1)
            par.set_user_params(L.USER_KIND_DYNAMICS, np.full((A, 1), 2.0, F))      # per agent, every row the same
            lit.set_dynamics_source(dl)
        np.testing.assert_allclose(par.evaluate(states, seq), lit.evaluate(states, seq), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("net", ["w4", "q4s", "pair", "xform"])
def test_learned_model_paths_match_the_literal_source(L, net):
    # w4: the 4-32-32-32-3 network's kernel; q4s: 26-200-200-20 at N <= 2048; pair: the same at N = 3000; xform: the
    # learned-model rollout compiled with a HipInverseTargetTransform and the reward inlined
    if net == "w4":
        S, U, dims, act, N, H = 3, 1, [4, 32, 32, 32, 3], [1, 1, 1, 0], 150, 15
    elif net == "xform":
        S, U, dims, act, N, H = 20, 6, [26, 200, 200, 20], [1, 1, 0], 300, 10
    else:
        S, U, dims, act, N, H = 20, 6, [26, 200, 200, 20], [1, 1, 0], 300 if net == "q4s" else 3000, 10
    A = 2
    ws, bs = O.make_mlp_params(dims, seed=42)
    stats = [np.zeros(S, F), np.ones(S, F), np.zeros(U, F), np.ones(U, F), np.zeros(S, F), np.full(S, 0.1, F)]
    goal = [0.25, -0.5, 0.0625]
    rp, rl = _forms(GOAL_REWARD, REWARD_SIG, goal)
    engines = []
    for src, npar in ((rp, 3), (rl, 0)):
        e = _engine(L, L.DYN_MLP, L.REW_USER, A, H, S=S, lo=[-1.0] * U, hi=[1.0] * U)
        e.set_mlp(ws, bs, act, stats)
        if net == "xform":
            e.set_inverse_transform_source(IDENTITY_XFORM)
        e.set_reward_source(src, npar)
        if npar:
            e.set_user_params(L.USER_KIND_REWARD, np.tile(np.asarray(goal, F), (A, 1)))
        engines.append(e)
    rng = np.random.default_rng(11)
    states = (O.pendulum_start_states(A) if S == 3 else O.cheetah_start_states(A, S))
    seq = rng.uniform(-1, 1, (N, A, H, U)).astype(F)
    got, want = engines[0].evaluate(states, seq), engines[1].evaluate(states, seq)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)


# ---- 2. per-agent goals and masses against NumPy ----------------------------------------------------------------------
def test_per_agent_goals_and_masses_against_numpy(L):
    A, H, N = 3, 10, 160
    goals = np.array([[0.5, 0.01], [-1.0, 0.02], [2.5, 0.001]], F)
    masses = np.array([[1.0], [2.0], [0.5]], F)
    rp, _ = _forms(ANGLE_REWARD, REWARD_SIG, [0, 0])
    dp, _ = _forms(MASS_PENDULUM, DYNAMICS_SIG, [0])
    rng = np.random.default_rng(5)
    states = O.pendulum_start_states(A)
    seq = rng.uniform(-2, 2, (N, A, H, 1)).astype(F)
    # goals over the built-in pendulum model
    eng = _engine(L, L.DYN_PENDULUM, L.REW_USER, A, H)
    eng.set_reward_source(rp, 2)
    eng.set_user_params(L.USER_KIND_REWARD, goals)
    got = eng.evaluate(states, seq)
    for a in range(A):
        ev = O.Evaluator(_np_angle_reward(*goals[a]), O.Handler(O.pendulum_dynamics, True))
        np.testing.assert_allclose(got[:, a:a + 1], ev(states[a:a + 1], seq[:, a:a + 1]), rtol=R_RTOL, atol=R_ATOL)
    # goals and masses, both user functions
    eng = _engine(L, L.DYN_USER, L.REW_USER, A, H)
    eng.set_reward_source(rp, 2)
    eng.set_dynamics_source(dp, 1)
    eng.set_user_params(L.USER_KIND_REWARD, goals)
    eng.set_user_params(L.USER_KIND_DYNAMICS, masses)
    got = eng.evaluate(states, seq)
    for a in range(A):
        ev = O.Evaluator(_np_angle_reward(*goals[a]), O.Handler(_np_mass_pendulum(masses[a, 0]), True))
        np.testing.assert_allclose(got[:, a:a + 1], ev(states[a:a + 1], seq[:, a:a + 1]), rtol=R_RTOL, atol=R_ATOL)
    # one-step calls: B / A consecutive rows per agent
    s = np.repeat(states, 2, axis=0)
    act = rng.uniform(-2, 2, (2 * A, 1)).astype(F)
    nxt = eng.predict_next_state(s, act)
    for a in range(A):
        rows = slice(2 * a, 2 * a + 2)
        x = np.concatenate([s[rows], act[rows]], axis=1)
        np.testing.assert_allclose(nxt[rows], (s[rows] + _np_mass_pendulum(masses[a, 0])(x)).astype(F), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(eng.evaluate_next_reward(s, nxt, act)[rows],
                                   _np_angle_reward(*goals[a])(s[rows], act[rows], nxt[rows]), rtol=1e-5, atol=1e-5)


# ---- 3. t reaches the function ------------------------------------------------------------------------------------------
def test_planning_step_indexes_a_reference_trajectory(L):
    A, H, N, S = 2, 8, 100, 3
    rng = np.random.default_rng(9)
    ref = rng.uniform(-1, 1, (A, H, S)).astype(F)
    eng = _engine(L, L.DYN_PENDULUM, L.REW_USER, A, H)
    eng.set_reward_source(TRACKING_REWARD, H * S)
    eng.set_user_params(L.USER_KIND_REWARD, ref.reshape(A, H * S))
    states = O.pendulum_start_states(A)
    seq = rng.uniform(-2, 2, (N, A, H, 1)).astype(F)
    got = eng.evaluate(states, seq)
    for a in range(A):
        x = np.repeat(states[a:a + 1], N, axis=0)
        total = np.zeros(N, F)
        for t in range(H):
            nxt = (x + O.pendulum_dynamics(np.concatenate([x, seq[:, a, t]], axis=1))).astype(F)
            d = (nxt - ref[a, t]).astype(F)
            total = (total - (d * d).sum(axis=1)).astype(F)
            x = nxt
        np.testing.assert_allclose(got[:, a], total, rtol=R_RTOL, atol=R_ATOL)
    # a one-step call is t = 0: the first reference state
    s, act = states, seq[0, :, 0]
    nxt = eng.predict_next_state(s, act)
    want = np.array([-((nxt[a] - ref[a, 0]) ** 2).sum() for a in range(A)], F)
    np.testing.assert_allclose(eng.evaluate_next_reward(s, nxt, act), want, rtol=1e-5, atol=1e-5)


# ---- 4. live updates without recompiling ------------------------------------------------------------------------------
def _policy(reward, opt_name, A, seed=21, **kw):
    from blackbox_mpc_amd.policies import MPCPolicy
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.utils.device_functions import HipDynamicsFunction
    return MPCPolicy(reward_function=reward, env_action_space=Box(LO, HI), env_observation_space=Box([-1, -1, -8], [1, 1, 8]),
                     true_model=True, dynamics_function=HipDynamicsFunction(USER_PENDULUM_MODEL), optimizer_name=opt_name,
                     num_agents=A, planning_horizon=10, population_size=160, max_iterations=3, seed=seed,
                     **dict({"num_elite": 16} if opt_name == "CEM" else {}, **kw))


def _goals_at(t, A):
    base = 0.5 if t < 5 else -1.25                           # the goal moves mid-episode
    return np.array([[base + 0.25 * a, 0.01] for a in range(A)], F)


@pytest.mark.parametrize("opt_name", ["CEM", "PI2"])
def test_live_updates_walk_in_step_with_a_torch_goal_and_never_recompile(L, opt_name):
    import torch
    from blackbox_mpc_amd.utils.device_functions import HipRewardFunction
    A = 2
    rp, _ = _forms(ANGLE_REWARD, REWARD_SIG, [0, 0])
    hip = HipRewardFunction(rp, num_params=2)
    goal = torch.zeros(A, device="cuda")

    def torch_reward(cur, act, nxt):
        g = goal.repeat_interleave(cur.shape[0] // A)       # rows b = a * (B / A) + n
        d = torch.atan2(nxt[:, 1], nxt[:, 0]) - g
        return -(d * d) - 0.01 * (act[:, 0] * act[:, 0])
    pol_h, pol_t = _policy(hip, opt_name, A), _policy(torch_reward, opt_name, A)
    eng = pol_h._optimizer._engine
    obs_h = obs_t = O.pendulum_start_states(A)
    compiles = None
    for t in range(10):
        g = _goals_at(t, A)
        hip.set_params(g)
        goal.copy_(torch.from_numpy(g[:, 0]))
        torch.cuda.synchronize()
        a_h, n_h, r_h = pol_h.act(obs_h, t)
        a_t, n_t, r_t = pol_t.act(obs_t, t)
        if compiles is None:
            compiles = eng.compile_count()                   # the sources and the lazily built rollout
        np.testing.assert_allclose(a_h, a_t, rtol=0, atol=5e-4)
        np.testing.assert_allclose(n_h, n_t, rtol=0, atol=1e-4)
        np.testing.assert_allclose(r_h, r_t, rtol=1e-4, atol=1e-4)
        obs_h, obs_t = n_h, n_t
    assert eng.compile_count() == compiles


# ---- 5. the record's reward uses each agent's own row -----------------------------------------------------------------
def test_record_reward_uses_each_agents_row(L):
    from blackbox_mpc_amd.utils.device_functions import HipRewardFunction
    from blackbox_mpc_amd.utils.rollouts import rollout_on_device
    A = 3
    rp, _ = _forms(ANGLE_REWARD, REWARD_SIG, [0, 0])
    hip = HipRewardFunction(rp, num_params=2)
    goals = np.array([[0.5, 0.01], [-2.0, 0.05], [1.5, 0.0]], F)
    hip.set_params(goals)
    pol = _policy(hip, "CEM", A)
    obs = O.pendulum_start_states(A)
    for t in range(2):
        a, n, r = pol.act(obs, t)
        for k in range(A):
            want = _np_angle_reward(*goals[k])(obs[k:k + 1], a[k:k + 1], n[k:k + 1])
            np.testing.assert_allclose(r[k:k + 1], want, rtol=1e-5, atol=1e-5)
        obs = n
    acts, obs_seq, rews = rollout_on_device(pol, O.pendulum_start_states(A), 4)
    for t in range(4):
        for k in range(A):
            want = _np_angle_reward(*goals[k])(obs_seq[t, k:k + 1], acts[t, k:k + 1], obs_seq[t + 1, k:k + 1])
            np.testing.assert_allclose(rews[t, k:k + 1], want, rtol=1e-5, atol=1e-5)


# ---- 6. agent shards --------------------------------------------------------------------------------------------------
def _in_threads(fns):
    out, err = [None] * len(fns), [None] * len(fns)

    def run(i):
        try:
            out[i] = fns[i]()
        except BaseException as ex:                           # noqa: BLE001
            err[i] = ex
    ts = [threading.Thread(target=run, args=(i,)) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not any(t.is_alive() for t in ts)
    for e in err:
        if e is not None:
            raise e
    return out


def test_agent_shards_use_their_own_rows(L):
    from blackbox_mpc_amd import parallel as P
    from blackbox_mpc_amd.utils.device_functions import HipRewardFunction
    A_glob, R = 4, 2
    rp, _ = _forms(ANGLE_REWARD, REWARD_SIG, [0, 0])
    hip = HipRewardFunction(rp, num_params=2)
    hip.set_params(_goals_at(0, A_glob))
    full = _policy(hip, "CEM", A_glob)
    shards = [P.agent_shard(A_glob, R, r) for r in range(R)]
    ranks = [_policy(hip, "CEM", cnt, agent_offset=off, num_agents_global=A_glob) for off, cnt in shards]
    obs = O.pendulum_start_states(A_glob)
    for t in range(4):
        hip.set_params(_goals_at(3 * t, A_glob))
        a_f, n_f, r_f = full.act(obs, t)

        def rank_step(r, t=t, obs=obs):
            off, cnt = shards[r]
            return ranks[r].act(obs[off:off + cnt], t)
        # the first step sequentially (each rank compiles its rollout), then a rank per host thread
        res = [rank_step(r) for r in range(R)] if t == 0 else _in_threads([lambda r=r: rank_step(r) for r in range(R)])
        a_g = np.concatenate([x[0] for x in res])
        n_g = np.concatenate([x[1] for x in res])
        r_g = np.concatenate([x[2] for x in res])
        np.testing.assert_allclose(a_g, a_f, rtol=0, atol=5e-4)
        np.testing.assert_allclose(n_g, n_f, rtol=0, atol=1e-4)
        np.testing.assert_allclose(r_g, r_f, rtol=1e-4, atol=1e-4)
        obs = n_f


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals(L):
    from blackbox_mpc_amd.dynamics_handlers import SystemDynamicsHandler
    from blackbox_mpc_amd.spaces import Box
    from blackbox_mpc_amd.trajectory_evaluators import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.device_functions import HipDynamicsFunction, HipRewardFunction
    A, H, P_ = 3, 5, 2
    rp, rl = _forms(ANGLE_REWARD, REWARD_SIG, [0.5, 0.01])
    states = O.pendulum_start_states(A)
    seq = np.zeros((16, A, H, 1), F)
    eng = _engine(L, L.DYN_PENDULUM, L.REW_USER, A, H)
    eng.set_reward_source(rp, P_)
    with pytest.raises(L.BBMPCError) as ei:                   # computing before the parameters were set
        eng.evaluate(states, seq)
    assert ei.value.code == L.E_STATE
    for bad in (np.zeros(P_ + 1, F), np.zeros((A - 1, P_), F), np.zeros((A + 1, P_), F)):
        with pytest.raises(L.BBMPCError) as ei:               # count neither P nor A * P
            eng.set_user_params(L.USER_KIND_REWARD, bad)
        assert ei.value.code == L.E_INVALID
    with pytest.raises(L.BBMPCError) as ei:                   # the dynamics are built in: nothing to parameterise
        eng.set_user_params(L.USER_KIND_DYNAMICS, np.zeros(P_, F))
    assert ei.value.code == L.E_STATE
    eng.set_user_params(L.USER_KIND_REWARD, np.zeros((A, P_), F))
    eng.evaluate(states, seq)
    s4 = np.repeat(states[:1], 4, axis=0)
    a4 = np.zeros((4, 1), F)
    with pytest.raises(L.BBMPCError) as ei:                   # 4 rows, 3 agents with rows of their own
        eng.evaluate_next_reward(s4, s4, a4)
    assert ei.value.code == L.E_INVALID
    eng.set_user_params(L.USER_KIND_REWARD, np.zeros(P_, F))  # shared parameters: any number of rows
    assert eng.evaluate_next_reward(s4, s4, a4).shape == (4,)
    classic = _engine(L, L.DYN_PENDULUM, L.REW_USER, A, H)
    classic.set_reward_source(rl)
    with pytest.raises(L.BBMPCError) as ei:
        classic.set_user_params(L.USER_KIND_REWARD, np.zeros(P_, F))
    assert ei.value.code == L.E_STATE
    # the same through the evaluator: per-agent parameters with 3 rows, a one-step call on 4 rows
    dyn = HipDynamicsFunction(_forms(MASS_PENDULUM, DYNAMICS_SIG, [1.0])[0], num_params=1)
    dyn.set_params(np.ones((A, 1), F))
    h = SystemDynamicsHandler(env_action_space=Box(LO, HI), env_observation_space=Box([-1, -1, -8], [1, 1, 8]),
                              true_model=True, dynamics_function=dyn)
    ev = DeterministicTrajectoryEvaluator(reward_function=HipRewardFunction(rl), system_dynamics_handler=h)
    assert ev.predict_next_state(np.repeat(states, 2, axis=0), np.zeros((2 * A, 1), F)).shape == (2 * A, 3)
    with pytest.raises(L.BBMPCError) as ei:
        ev.predict_next_state(s4, a4)
    assert ei.value.code == L.E_INVALID
