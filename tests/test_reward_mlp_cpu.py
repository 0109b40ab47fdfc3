"""Learned reward models without a GPU: the float64 NumPy statement of the scorer (tests/reward_mlp_util.py) on
hand-computed values, the LearnedRewardMLP container, and the conditioning of the GPU tests' networks -- every indexing
slip the device code could make must move the statement's result by far more than the tolerance the GPU tests compare with."""
import numpy as np
import pytest

from tests import reward_mlp_util as R

F = np.float32


def test_statement_on_hand_computed_values():
    # 2 layers, S = 1, U = 1, inputs (s_t, a_t, s_{t+1}); statistics chosen so that every step is exact by hand
    net = R.Net("hand", 1, 1, 7, [2], ["relu", None], True, 0)
    net.ws = [np.array([[1.0, -1.0], [0.5, 0.0], [0.0, 2.0]], F), np.array([[2.0], [-1.0]], F)]
    net.bs = [np.array([0.0, 1.0], F), np.array([0.5], F)]
    net.stats = [np.array([1.0, 0.0, -1.0], F), np.array([2.0, 1.0, 0.5], F), np.array([10.0], F), np.array([3.0], F)]
    # row: s_t = 3, a_t = 2, s_{t+1} = 0  ->  x = ((3-1)/2, (2-0)/1, (0+1)/0.5) = (1, 2, 2) (up to the 1e-7 in the divisor)
    # layer 0: (1*1 + 2*0.5 + 2*0, 1*-1 + 2*0 + 2*2 + 1) = (2, 4) -> relu (2, 4);  layer 1: 2*2 - 4 + 0.5 = 0.5
    # r = 0.5 * 3 + 10 = 11.5
    r = net.rows([[3.0]], [[2.0]], [[0.0]])
    np.testing.assert_allclose(r, [11.5], rtol=0, atol=1e-5)
    # second row flips the first relu off: s_t = -3 -> x0 = -2: layer 0 = (-2 + 1, 2 + 4 + 1) = (-1, 7) -> (0, 7); y = -6.5; r = -9.5
    r2 = net.rows([[-3.0]], [[2.0]], [[0.0]])
    np.testing.assert_allclose(r2, [-9.5], rtol=0, atol=1e-5)
    # the sum runs over t, NaN -> -1e6 per trajectory
    steps = np.array([[11.5, -9.5], [np.nan, 1.0]])
    np.testing.assert_array_equal(R.returns(steps), [2.0, -1.0e6])
    # per_step: current state of step t is the start state at t = 0 and the previous next state afterwards
    got = R.per_step(net, np.array([[3.0]]), np.array([[[0.0], [5.0]]]), np.array([[[2.0], [1.0]]]))
    np.testing.assert_allclose(got[0, 0], 11.5, atol=1e-5)
    np.testing.assert_allclose(got[0, 1], net.rows([[0.0]], [[1.0]], [[5.0]])[0], atol=0)


def test_mask_selects_and_orders_the_blocks():
    net = R.small_nets()[3]                                  # inputs (s_t, a_t)
    cur, act, nxt = np.arange(3.0)[None], np.array([[7.0]]), np.full((1, 3), 99.0)
    np.testing.assert_array_equal(net.assemble(cur, act, nxt), [[0.0, 1.0, 2.0, 7.0]])
    net4 = R.small_nets()[4]                                 # s_{t+1} alone
    np.testing.assert_array_equal(net4.assemble(cur, act, nxt), [[99.0, 99.0, 99.0]])


def test_learned_reward_mlp_call_statistics_save_load(tmp_path):
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP, input_mask
    assert [input_mask(s) for s in ("sas", "sa", "s'", "s", "as", "ss'", "a")] == [7, 3, 4, 1, 6, 5, 2]
    with pytest.raises(ValueError):
        input_mask("sx")
    with pytest.raises(ValueError):
        LearnedRewardMLP(3, 1, [20, 2], ["tanh", None])
    for net in R.small_nets():
        m = LearnedRewardMLP(net.S, net.U, net.dims[1:], net.acts, inputs=net.mask)
        assert m._bbmpc_reward_kind == L.REW_MLP and m.input_mask == net.mask and m.dim_in == net.D
        assert m.activation_codes == net.codes() and m.normalization_stats() is None
        v0 = m._version
        m.set_weights(net.ws, net.bs)
        m.set_normalization_stats(net.stats)
        assert m._version > v0
        start, states, actions = R.random_trajectories(net, 9, 1, 3)
        want = net.rows(start, actions[:, 0], states[:, 0])
        got = m(start.astype(F), actions[:, 0].astype(F), states[:, 0].astype(F))
        assert got.dtype == F
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
        path = str(tmp_path / (net.name + ".npz"))
        m.save(path)
        m2 = LearnedRewardMLP.load(path)
        assert m2.input_mask == m.input_mask and m2.layer_sizes == m.layer_sizes and m2.activation_codes == m.activation_codes
        np.testing.assert_array_equal(m2(start.astype(F), actions[:, 0].astype(F), states[:, 0].astype(F)), got)
        assert (m2.normalization_stats() is None) == (net.stats is None)


def test_train_fits_a_linear_target_on_cpu_torch():
    pytest.importorskip("torch")
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    rng = np.random.default_rng(0)
    S, U, B = 3, 1, 2048
    s, a, n = rng.normal(1.0, 2.0, (B, S)).astype(F), rng.uniform(-2, 2, (B, U)).astype(F), rng.normal(0, 1, (B, S)).astype(F)
    coef = np.array([0.5, -1.0, 2.0, 3.0, 0.25, 0.0, -0.75])
    r = (np.concatenate([s, a, n], 1) @ coef + 4.0).astype(F)
    m = LearnedRewardMLP(S, U, [1], [None], inputs="sas", seed=1)
    v0 = m._version
    tl, vl = m.train(s, a, n, r, epochs=60, batch_size=64, learning_rate=2e-2, validation_split=0.2, device="cpu", seed=5)
    assert m._version > v0 and m.normalization_stats() is not None
    assert tl[-1] < 1e-3 * tl[0] and vl[-1] < 1e-3
    err = np.abs(m(s, a, n) - r)
    assert err.max() < 0.05 * r.std(), err.max()


# ---- input conditioning: asserted on the statement alone ------------------------------------------------------------
LO, HI = np.array([0.25]), np.array([0.75])                  # tests/bounds_util.NARROW, the GPU test's bounds at U = 1


def _nets():
    return R.small_nets() + [R.medium_net(), R.limits_net()]


def _moves(a, b, rtol, atol):
    """largest change over the rows in units of the comparison tolerance at that row"""
    return float(np.max(np.abs(a - b) / (atol + rtol * np.abs(a))))


@pytest.mark.parametrize("net", _nets(), ids=lambda n: n.name)
def test_input_conditioning(net):
    """Each slip must move the float64 result by more than 100 x the tolerance its GPU comparison uses: the per-step
    rewards (rewards_out, evaluate_next_reward: rtol 2e-5 + atol 2e-5) for the slips inside a row, the H-step returns
    (evaluate, the traces: rtol 1e-3 + atol 1e-3 H) for the slips of the trajectory frame."""
    B, Hq = (16, 2) if net.D == 192 else (37, 5)
    lo, hi = (LO, HI) if net.U == 1 else (-0.5 * np.ones(net.U), 0.5 * np.ones(net.U))
    start, states, raw = R.random_trajectories(net, B, Hq, 21, lo, hi)
    actions = np.clip(raw, lo, hi)
    assert np.any(raw < lo) and np.any(raw > hi)
    base = R.per_step(net, start, states, actions)
    rt, at = R.ONE_STEP
    cur = np.concatenate([start[:, None], states[:, :-1]], 1)
    flat = lambda x: x.reshape(B * Hq, -1)
    # swapping the s_t and s_{t+1} blocks
    swapped = net.rows(flat(states), flat(actions), flat(cur)).reshape(B, Hq)
    assert _moves(base, swapped, rt, at) > 100
    # dropping the last input column
    ws = [net.ws[0].copy()] + net.ws[1:]
    ws[0][-1, :] = 0
    assert _moves(base, R.per_step(net, start, states, actions, ws=ws), rt, at) > 100
    # dropping the last hidden unit (of every hidden layer in turn)
    for l in range(len(net.ws) - 1):
        ws = [w.copy() for w in net.ws]
        ws[l + 1][-1, :] = 0
        assert _moves(base, R.per_step(net, start, states, actions, ws=ws), rt, at) > 100, l
    # the trajectory frame: t shifted by one, the unclipped action
    total = R.returns(base)
    h_rt, h_at = R.H_STEP_RTOL, R.H_STEP_ATOL_PER_STEP * Hq
    shifted = R.per_step(net, states[:, 0], np.concatenate([states[:, 1:], states[:, -1:]], 1), actions)      # rows of t + 1
    assert _moves(total, R.returns(shifted), h_rt, h_at) > 100
    if net.mask & 2:
        unclipped = R.per_step(net, start, states, raw)
        assert _moves(total, R.returns(unclipped), h_rt, h_at) > 100
        assert _moves(base, unclipped, rt, at) > 100
