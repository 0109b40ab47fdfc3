"""CPU tests of the learned policy prior: the LearnedPolicyMLP container, the float64 statement and
`PriorCEM` of tests/policy_prior_util.py, the restatement of noise stream 12, and the constructor errors of CEMOptimizer."""
import numpy as np
import pytest

from oracle import oracle_np as O
from tests import elite_carry_util as EC
from tests import policy_prior_util as PP

F = np.float32
S, U = 3, 1


def _policy_class():
    from blackbox_mpc_amd.policy_functions.learned_policy_mlp import LearnedPolicyMLP
    return LearnedPolicyMLP


# ---- 1. the container --------------------------------------------------------------------------------------------------
def test_container_round_trip(tmp_path):
    P = _policy_class()
    m = P(5, 2, [24, 8, 2], ["swish", "tanh", None], seed=3)
    assert m.layer_sizes == [5, 24, 8, 2] and m._version == 0
    rng = np.random.default_rng(0)
    m.set_normalization_stats((rng.normal(0, 1, 5), rng.uniform(0.5, 2, 5), rng.normal(0, 1, 2), rng.uniform(0.5, 2, 2)))
    assert m._version == 1
    m.save(str(tmp_path / "pi.npz"))
    z = P.load(str(tmp_path / "pi.npz"))
    assert z.layer_sizes == m.layer_sizes and z.activation_codes == m.activation_codes
    for a, b in zip(m.weights + m.biases + list(m.normalization_stats()), z.weights + z.biases + list(z.normalization_stats())):
        np.testing.assert_array_equal(a, b)
    x = rng.normal(0, 1, (7, 5))
    np.testing.assert_array_equal(m(x), z(x))
    v = m._version
    m.set_weights(m.weights, m.biases)
    assert m._version == v + 1                              # every engine that holds it uploads it again
    with pytest.raises(ValueError):
        P(5, 2, [24, 3], ["tanh", None])                    # does not end in dim_U
    with pytest.raises(ValueError):
        P(5, 2, [24, 2], ["tanh"])
    with pytest.raises(ValueError):
        m.set_normalization_stats((np.zeros(5), np.ones(5), np.zeros(1), np.ones(2)))


@pytest.mark.parametrize("normalized", [True, False])
def test_numpy_call_is_the_float64_statement(normalized):
    P = _policy_class()
    net = PP.PolicyNet("swish24-tanh8", 5, 2, [24, 8], ["swish", "tanh", None], normalized, 31)
    m = P(5, 2, [24, 8, 2], ["swish", "tanh", None])
    m.set_weights(net.ws, net.bs)
    m.set_normalization_stats(net.stats)
    x = np.random.default_rng(1).normal(0, 1, (33, 5))
    got, want = m(x), net(x)
    assert got.dtype == np.float32 and got.shape == (33, 2)
    np.testing.assert_array_equal(got, want.astype(F))      # float64 throughout, one rounding at the end


def test_train_reduces_the_loss_on_a_linear_policy():
    P = _policy_class()
    rng = np.random.default_rng(2)
    gain = rng.normal(0, 1, (4, 2))
    x = rng.normal(0, 1, (600, 4)).astype(F)
    y = (x @ gain + 0.3).astype(F)
    m = P(4, 2, [2], [None], seed=5)
    before = float(np.mean((m(x) - y) ** 2))
    v = m._version
    trn, val = m.train(x, y, epochs=40, batch_size=64, learning_rate=1e-2, device="cpu", seed=0)
    after = float(np.mean((m(x) - y) ** 2))
    print("policy regression: mse %.4f -> %.5f, train loss %.4f -> %.5f" % (before, after, trn[0], trn[-1]))
    assert trn[-1] < 0.1 * trn[0] and after < 0.1 * before
    assert m._version > v and m.normalization_stats() is not None
    # train_on_rollouts: observations [T+1, A, S], executed actions [T, A, U]
    obs = rng.normal(0, 1, (11, 3, 4)).astype(F)
    acs = (obs[:10] @ gain + 0.3).astype(F)
    m.train_on_rollouts([obs], [acs], epochs=2, device="cpu", seed=0)
    assert m._pairs[0][0].shape == (30, 4) and m._pairs[0][1].shape == (30, 2)


# ---- 2. the rule -------------------------------------------------------------------------------------------------------
N, A, H, K_EL, ITERS = 24, 2, 4, 5, 3


def _setup(seed=0):
    dims = [S + U, 12, S]
    ws, bs = O.make_mlp_params(dims, seed=seed)
    rng = np.random.default_rng(seed + 1)
    stats = [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F), rng.normal(0, 0.1, U).astype(F),
             rng.uniform(0.5, 1.5, U).astype(F), rng.normal(0, 0.01, S).astype(F), rng.uniform(0.05, 0.15, S).astype(F)]
    handler = O.Handler(O.MLP(ws, bs, ["tanh", None]), False, True, stats)
    ev = O.Evaluator("pendulum", handler)
    pol = PP.PolicyNet("tanh8", S, U, [8], ["tanh", None], True, 22)
    states = O.pendulum_start_states(A)
    lo, hi = [-1.0] * U, [1.0] * U
    noise = {"trunc": [O.truncated_normal_noise(rng, (N, A, H, U)) for _ in range(ITERS)],
             "policy": [rng.standard_normal((A, 3, H, U)).astype(F) for _ in range(ITERS)]}
    return ev, handler, pol, states, lo, hi, noise


def test_free_running_statement_is_its_own_teacher_forced_one():
    ev, handler, pol, states, lo, hi, noise = _setup()
    xi = noise["policy"][0]
    acts, sts = PP.policy_rollouts64(pol, handler, states, xi, 0.3, lo, hi)
    assert acts.shape == (3, A, H, U) and sts.shape == (3, A, H, S)
    assert np.all(acts >= -1.0) and np.all(acts <= 1.0)
    for e in range(3):
        for a in range(A):
            s = states[a].astype(np.float64)
            for t in range(H):
                at = PP.policy_action64(pol, s[None], xi[a, e, t][None], 0.3, lo, hi)[0]
                # (float64 products of one row and of a batch may be summed in another order: a few ulp of float64)
                np.testing.assert_allclose(at, acts[e, a, t], rtol=1e-12, atol=1e-12)
                s = PP.model_step64(handler, s[None], at[None])[0]
                np.testing.assert_allclose(s, sts[e, a, t], rtol=1e-12, atol=1e-12)
    # the float64 model step is the oracle's float32 one up to float32 rounding
    nxt32 = ev.predict_next_state(np.tile(states, (3, 1)), acts[:, :, 0].reshape(3 * A, U).astype(F))
    np.testing.assert_allclose(nxt32, sts[:, :, 0].reshape(3 * A, S), rtol=1e-5, atol=1e-5)
    # sigma = 0, K = 1: the deterministic rollout, whatever the noise
    d0, _ = PP.policy_rollouts64(pol, handler, states, xi[:, :1], 0.0, lo, hi)
    d1, _ = PP.policy_rollouts64(pol, handler, states, np.zeros_like(xi[:, :1]), 0.0, lo, hi)
    np.testing.assert_array_equal(d0, d1)


def _rollouts(pol, handler, sigma, lo, hi):
    return lambda state, xi: PP.policy_rollouts64(pol, handler, state, xi, sigma, lo, hi)[0]


def test_prior_cem_on_the_plain_optimizer_places_the_columns():
    ev, handler, pol, states, lo, hi, noise = _setup()
    K = 3
    kw = dict(horizon=H, max_iterations=ITERS, population=N, num_elite=K_EL, num_agents=A)
    plain = O.CEM(ev, lo, hi, **kw)
    prior = PP.PriorCEM(ev, lo, hi, count=K, rollouts=_rollouts(pol, handler, 0.3, lo, hi), **kw)
    plain._optimize(states, noise)
    prior._optimize(states, noise)
    assert prior.columns == [(N - K, 0)] * ITERS
    # iteration 0 samples from the same distribution: every other column keeps oracle_np.CEM's bits
    np.testing.assert_array_equal(prior.trace[0]["samples"][:N - K], plain.trace[0]["samples"][:N - K])
    for it in range(ITERS):
        want = PP.policy_rollouts64(pol, handler, states, noise["policy"][it], 0.3, lo, hi)[0].astype(F)
        np.testing.assert_array_equal(prior.trace[it]["samples"][N - K:], want)
    assert not np.array_equal(prior.trace[0]["samples"][N - K:], plain.trace[0]["samples"][N - K:])
    # the rewards of the policy columns are the evaluator's on those sequences
    np.testing.assert_array_equal(prior.trace[0]["rewards"][N - K:], ev(states, prior.trace[0]["samples"][N - K:]))


def test_prior_cem_on_carry_cem_keeps_the_column_order():
    ev, handler, pol, states, lo, hi, noise = _setup(seed=4)
    K, keep, shift = 3, 2, 1
    kw = dict(horizon=H, max_iterations=ITERS, population=N, num_elite=K_EL, num_agents=A)
    prior = PP.PriorCEM(ev, lo, hi, count=K, rollouts=_rollouts(pol, handler, 0.0, lo, hi), keep=keep, shift=shift, **kw)
    prior._optimize(states, noise)
    first = [dict(t) for t in prior.trace]
    assert prior.columns == [(N - K, 0), (N - keep - K, keep), (N - keep - K, keep)]
    assert prior.stored.shape == (shift, A, H, U)
    prior._optimize(states, noise)
    assert prior.columns == [(N - shift - K, shift), (N - keep - K, keep), (N - keep - K, keep)]
    second = prior.trace
    want = PP.policy_rollouts64(pol, handler, states, noise["policy"][0], 0.0, lo, hi)[0].astype(F)
    for it, (col0, c_i) in enumerate(prior.columns):
        np.testing.assert_array_equal(second[it]["samples"][col0:col0 + K], want)       # sigma = 0: every iteration's columns
    # the carried columns stay where section 8h puts them
    np.testing.assert_array_equal(second[0]["samples"][N - shift:],
                                  EC.shift_rows(EC.gather_elites(first[-1]["samples"], first[-1]["elites"], shift)))
    for it in range(1, ITERS):
        np.testing.assert_array_equal(second[it]["samples"][N - keep:],
                                      EC.gather_elites(second[it - 1]["samples"], second[it - 1]["elites"], keep))
    # and every other column of iteration 0 is the carry optimizer's without the prior, bit for bit
    twin = EC.CarryCEM(ev, lo, hi, keep=keep, shift=shift, **kw)
    twin._optimize(states, noise)
    np.testing.assert_array_equal(first[0]["samples"][:N - K], twin.trace[0]["samples"][:N - K])
    with pytest.raises(AssertionError):
        PP.PriorCEM(ev, lo, hi, count=N - keep, rollouts=None, keep=keep, shift=shift, **kw)


# ---- 3. stream 12 ------------------------------------------------------------------------------------------------------
def _philox_scalar(c, k):
    """Philox4x32-10 on Python ints, written out from the algorithm's definition (independent of tests/philox_np.py)"""
    c, k = list(c), list(k)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def test_stream_12_restatement_and_known_answer():
    import math
    seed, step, it, A_, K, H_, U_, off = 0x1234567890ABCDEF, 3, 1, 2, 3, 5, 3, 5        # H * U = 15: a ragged last block
    z = PP.policy_noise_np(seed, step, it, A_, K, H_, U_, agent_offset=off)
    assert z.shape == (A_, K, H_, U_) and np.all(np.isfinite(z))
    Qk = (H_ * U_ + 3) // 4
    for (a, e, t, u) in [(0, 0, 0, 0), (1, 2, 4, 2), (1, 1, 2, 1), (0, 2, 3, 0)]:
        j = t * U_ + u
        w = _philox_scalar([e, (off + a) * Qk + (j >> 2), step, (12 << 16) | it], [seed & 0xFFFFFFFF, seed >> 32])
        pair = (j & 3) >> 1
        u1 = ((w[2 * pair] >> 9) + 0.5) * 2.0 ** -23
        u2 = ((w[2 * pair + 1] >> 9) + 0.5) * 2.0 ** -23
        r = math.sqrt(-2.0 * math.log(u1))
        want = r * (math.cos(2.0 * math.pi * u2) if (j & 1) == 0 else math.sin(2.0 * math.pi * u2))
        assert abs(z[a, e, t, u] - want) <= 1e-12
    # the Philox4x32-10 known-answer vector of the Random123 distribution (counter and key of all ones' complement)
    assert _philox_scalar([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    # one element by hand: seed 0, step 0, iteration 0, agent 0, rollout 0, element 0 -- counter (0, 0, 0, 12 << 16), key (0, 0)
    w = _philox_scalar([0, 0, 0, 12 << 16], [0, 0])
    u1, u2 = ((w[0] >> 9) + 0.5) * 2.0 ** -23, ((w[1] >> 9) + 0.5) * 2.0 ** -23
    z0 = PP.policy_noise_np(0, 0, 0, 1, 1, 1, 1)[0, 0, 0, 0]
    assert abs(z0 - math.sqrt(-2.0 * math.log(u1)) * math.cos(2.0 * math.pi * u2)) <= 1e-12
    assert abs(z0 - KNOWN_Z0) <= 1e-9
    # another stream, another draw; rollouts and agents are independent counters
    assert not np.allclose(z, PP.policy_noise_np(seed, step, it + 1, A_, K, H_, U_, agent_offset=off))
    np.testing.assert_array_equal(z[1], PP.policy_noise_np(seed, step, it, 1, K, H_, U_, agent_offset=off + 1)[0])


# worked once by hand: Philox4x32-10 of counter (0, 0, 0, 0x000C0000) under key (0, 0) gives the words 0x7A45C556,
# 0x9A39F167, ...; u1 = ((w0 >> 9) + 0.5) 2^-23 = 0.47762709856, u2 = 0.60244661570; sqrt(-2 ln u1) cos(2 pi u2)
KNOWN_Z0 = -0.9723962429452025


# ---- 4. the Python surface ---------------------------------------------------------------------------------------------
def _spaces():
    from blackbox_mpc_amd import Box
    return Box(low=[-2.0], high=[2.0]), Box(low=[-1.0, -1.0, -8.0], high=[1.0, 1.0, 8.0])


def test_cem_optimizer_constructor_errors():
    from blackbox_mpc_amd.optimizers import CEMOptimizer
    act, obs = _spaces()
    pol = _policy_class()(3, 1, [8, 1], ["tanh", None], seed=0)
    kw = dict(planning_horizon=5, max_iterations=2, population_size=20, num_elite=4, num_agents=1)
    opt = CEMOptimizer(act, obs, policy_prior=pol, prior_candidates=3, prior_std=0.1, **kw)
    assert opt._policy_prior == (pol, 3, 0.1)
    assert CEMOptimizer(act, obs, **kw)._policy_prior is None
    for bad in (dict(policy_prior=pol, prior_candidates=0), dict(policy_prior=pol, prior_candidates=-1),
                dict(policy_prior=pol, prior_candidates=2.5), dict(policy_prior=pol, prior_candidates=True),
                dict(policy_prior=pol, prior_candidates=3, prior_std=-0.1),
                dict(policy_prior=pol, prior_candidates=3, prior_std=float("nan")),
                dict(policy_prior=pol, prior_candidates=3, prior_std=float("inf")),
                dict(policy_prior=pol, prior_candidates=20), dict(policy_prior=pol, prior_candidates=17, keep_elites=3),
                dict(policy_prior=pol, prior_candidates=17, shift_elites=3), dict(prior_candidates=3)):
        with pytest.raises(ValueError):
            CEMOptimizer(act, obs, **bad, **kw)
    with pytest.raises(TypeError):
        CEMOptimizer(act, obs, policy_prior=object(), prior_candidates=3, **kw)
    CEMOptimizer(act, obs, policy_prior=pol, prior_candidates=16, keep_elites=3, **kw)           # 16 + 3 < 20


@pytest.mark.parametrize("name", ["PI2Optimizer", "RandomSearchOptimizer", "PSOOptimizer", "SPSAOptimizer", "CMAESOptimizer"])
def test_other_optimizers_raise_type_error(name):
    from blackbox_mpc_amd import optimizers
    act, obs = _spaces()
    pol = _policy_class()(3, 1, [8, 1], ["tanh", None], seed=0)
    with pytest.raises(TypeError):
        getattr(optimizers, name)(act, obs, planning_horizon=5, num_agents=1, policy_prior=pol, prior_candidates=3)
