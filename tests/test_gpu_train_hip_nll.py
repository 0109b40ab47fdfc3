"""The Gaussian-NLL instantiations of the training kernels on the GPU (HipGaussianTrainer,
HipGaussianEnsembleTrainer, backend="hip_nll"): gradients against the float64 rule with the torch DenseTrainer's own error as
the yardstick, whole fits at the project's fit tolerances, bit reproducibility and member = single trainer, weight decay and
early stopping on the head, refusals and lifecycle, and the package's paths."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle_np as O
from oracle import oracle_train as OT
from tests import train_hip_util as U
from tests import train_nll_util as N
from tests.test_gpu_activations import CODE
from tests.test_train_cpu import _episodes

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_ATOL, LOSS_RTOL, LOSS_ATOL = 3e-4, 2e-4, 1e-6          # tests/test_gpu_train.py's


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _trainer(ws, bs, acts, head, **kw):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipGaussianTrainer
    return HipGaussianTrainer(ws, bs, [CODE[a] for a in acts], None, logvar_head=head, **kw)


def _ensemble(members, acts, heads, **kw):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipGaussianEnsembleTrainer
    return HipGaussianEnsembleTrainer([m[0] for m in members], [m[1] for m in members], [CODE[a] for a in acts], None,
                                      logvar_heads=[h[:2] for h in heads], min_logvar=heads[0][2], max_logvar=heads[0][3], **kw)


def _params(tr, member=None):
    """Weights, biases and the head, one list."""
    w, b = tr.numpy_params() if member is None else tr.numpy_params(member)
    return w + b + list(tr.numpy_logvar_head() if member is None else tr.numpy_logvar_head(member))


# ---- 1. gradients -----------------------------------------------------------------------------------------------------
def _torch_gradients(ws, bs, codes, head, x, y):
    """DenseTrainer's gradient of the batch, rebuilt the way DenseTrainer._step does (head included)."""
    import torch
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer, _act_grad
    tr = DenseTrainer(ws, bs, codes, "cuda", logvar_head=head)
    xt, yt = torch.as_tensor(x).to(tr.dev), torch.as_tensor(y).to(tr.dev)
    zs = []
    ys = tr.forward(xt, zs)
    diff = ys[-1] - yt
    n = len(tr.w)
    lv, dlv_dz = tr.logvar(ys[n - 1])
    inv = (-lv).exp()
    wsq = diff * diff * inv
    g = diff * inv * (2.0 / diff.numel())
    gz = (1.0 - wsq) * dlv_dz * (1.0 / diff.numel())
    gw, gb = [None] * n, [None] * n
    for l in reversed(range(n)):
        g = _act_grad(tr.acts[l], ys[l + 1], g, zs[l])
        gw[l] = ys[l].t() @ g
        gb[l] = g.sum(dim=0)
        if l:
            g = g @ tr.w[l].t()
            if l == n - 1:
                g = g + gz @ tr.wv.t()
    out = gw + gb + [ys[n - 1].t() @ gz, gz.sum(dim=0)]
    return float((wsq + lv).mean().item()), [t.cpu().numpy() for t in out]


_ORACLE = {}


def _oracle(net, B):
    """The case and its float64 truth, computed once."""
    if (net, B) not in _ORACLE:
        ws, bs, acts, head, x, y, idx = N.gradient_case(net, B)
        _ORACLE[net, B] = ((ws, bs, acts, head, x, y, idx), N.nll_and_grads(ws, bs, acts, head, x[idx], y[idx]))
    return _ORACLE[net, B]


@pytest.mark.parametrize("B", N.GRAD_BATCHES)
@pytest.mark.parametrize("net", sorted(N.NETS))
def test_gradients_against_the_float64_rule(L, net, B, capsys):
    """Per tensor, W_v and b_v included: err_hip <= max(4 err_torch, 1e-6), err = max|got - want| / max|want| -- the margin
    and the floor test_gradients_against_the_float64_oracle gives the MSE kernels."""
    (ws, bs, acts, head, x, y, idx), (want_loss, ww, wb, wwv, wbv) = _oracle(net, B)
    tr = _trainer(ws, bs, acts, head)
    tr.set_data(x, y, x[:0], y[:0])
    loss, gw, gb, gwv, gbv = tr.gradients(idx)
    t_loss, tg = _torch_gradients(ws, bs, [CODE[a] for a in acts], head, x[idx], y[idx])
    n = len(ws)
    names = ["W%d" % l for l in range(n)] + ["b%d" % l for l in range(n)] + ["Wv", "bv"]
    rows = [(name, U.rel_err(got, want), U.rel_err(tor, want))
            for name, got, tor, want in zip(names, gw + gb + [gwv, gbv], tg, ww + wb + [wwv, wbv])]
    with capsys.disabled():
        print("\n[train_hip_nll] gradient error %s B=%d (max|got-want|/max|want|; hip / torch): %s; loss %.3e / %.3e"
              % (net, B, ", ".join("%s %.2e / %.2e" % r for r in rows), abs(loss - want_loss) / abs(want_loss),
                 abs(t_loss - want_loss) / abs(want_loss)))
    for name, e_hip, e_torch in rows:
        assert e_hip <= max(4.0 * e_torch, 1e-6), (name, e_hip, e_torch)
    assert abs(loss - want_loss) <= max(4.0 * abs(t_loss - want_loss), 1e-6 * abs(want_loss))
    for got, start in zip(_params(tr), ws + bs + [head[0], head[1]]):      # nothing was updated
        np.testing.assert_array_equal(got, start)
    assert len(gw) == n and gwv.shape == head[0].shape and gbv.shape == head[1].shape


# ---- 2. whole fits ----------------------------------------------------------------------------------------------------
def _torch_fit(ws, bs, acts, head, tin, tout, vin, vout, perms, B, **kw):
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    tr = DenseTrainer(ws, bs, [CODE[a] for a in acts], "cuda", logvar_head=head, **kw)
    tr.fit(tin, tout, vin, vout, len(perms), B, permutations=perms)
    return tr.numpy_params()[0] + tr.numpy_params()[1] + list(tr.numpy_logvar_head())


def _assert_fit(got_params, losses, want, torch_params=None):
    w, b, hv, tl, vl = want[:5]
    truth = w + b + list(hv)
    for i, (got, ref) in enumerate(zip(got_params, truth)):
        bound = W_ATOL if torch_params is None else max(4.0 * float(np.max(np.abs(torch_params[i] - ref))), W_ATOL)
        assert float(np.max(np.abs(got - ref))) <= bound, (i, float(np.max(np.abs(got - ref))), bound)
    np.testing.assert_allclose(losses[0], tl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(losses[1], vl, rtol=LOSS_RTOL, atol=LOSS_ATOL)       # NaN == NaN here


@pytest.mark.parametrize("rule,lr", N.FIT_RULES)
@pytest.mark.parametrize("net", N.FIT_NETS)
def test_fit_matches_the_float64_rule(L, net, rule, lr):
    """Per tensor max|hip - f64| <= max(4 max|torch - f64|, 3e-4); losses at rtol 2e-4 / atol 1e-6."""
    ws, bs, acts, head, tin, tout, vin, vout, perms = N.fit_case(net, seed=20)
    tr = _trainer(ws, bs, acts, head, learning_rate=lr, rule=rule)
    losses = tr.fit(tin, tout, vin, vout, N.FIT_EPOCHS, N.FIT_BATCH, permutations=perms)
    want = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, learning_rate=lr, rule=rule)
    tor = _torch_fit(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, learning_rate=lr, rule=rule)
    _assert_fit(_params(tr), losses, want, tor)
    assert np.all(np.isfinite(losses[1])) and tr.epochs_run == N.FIT_EPOCHS and tr.best_epoch == -1
    d = vout.astype(np.float64) - U.forward(want[0], want[1], acts, vin)[0][-1]     # the mean network's residual
    np.testing.assert_allclose(tr.residual_rms(vin, vout), np.sqrt(np.mean(d * d, axis=0)), rtol=1e-4, atol=1e-6)


def test_validation_nll_is_nan_without_a_full_batch(L):
    ws, bs, acts, head, tin, tout, vin, vout, perms = N.fit_case("4-16-16-3", seed=40, n_val=20)
    tr = _trainer(ws, bs, acts, head, learning_rate=2e-3)
    losses = tr.fit(tin, tout, vin, vout, N.FIT_EPOCHS, N.FIT_BATCH, permutations=perms)
    want = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, learning_rate=2e-3)
    assert np.all(np.isnan(want[4])) and np.all(np.isnan(losses[1]))
    _assert_fit(_params(tr), losses, want)


# ---- 3. bits ----------------------------------------------------------------------------------------------------------
def test_equal_fits_give_equal_bits(L):
    ws, bs, acts, head, tin, tout, vin, vout, perms = N.fit_case("7-20-33-5", seed=60)
    runs = []
    for _ in range(2):
        tr = _trainer(ws, bs, acts, head)
        tl, vl = tr.fit(tin, tout, vin, vout, N.FIT_EPOCHS, N.FIT_BATCH, permutations=perms)
        runs.append(_params(tr) + [tl, vl])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(runs[0][-3], head[0])                         # the head moved


@pytest.mark.parametrize("E", [2, 3, 8])
def test_a_member_is_the_single_gaussian_trainer_bit_for_bit(L, E):
    """Weights, head and losses of member e = a HipGaussianTrainer with its start parameters on train[rows[e]] with its
    permutations -- also when another member holds NaN weights."""
    net = "7-20-33-5"
    dims, acts = N.NETS[net]
    _, _, _, head0, tin, tout, vin, vout, _ = N.fit_case(net, seed=70)
    rng = np.random.default_rng(71)
    n, epochs = tin.shape[0], 2
    members = [U.params(dims, seed=72 + e) for e in range(E)]
    heads = [(N.gauss_head(members[e][0], members[e][1], acts, tin, seed=90 + e)[:2] + head0[2:]) for e in range(E)]
    rows = [rng.integers(0, n, size=n) for _ in range(E)]
    perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(E)]
    singles = []
    for e in range(E):
        tr = _trainer(members[e][0], members[e][1], acts, heads[e], learning_rate=2e-3)
        tl, vl = tr.fit(tin[rows[e]], tout[rows[e]], vin, vout, epochs, N.FIT_BATCH, permutations=perms[e])
        singles.append(_params(tr) + [tl, vl])
    for poison in (None, E - 1):
        start = [(list(w), list(b)) for w, b in members]
        if poison is not None:
            start[poison] = ([np.full_like(w, np.nan) for w in members[poison][0]], members[poison][1])
        ens = _ensemble(start, acts, heads, learning_rate=2e-3)
        tl, vl = ens.fit(tin, tout, vin, vout, epochs, N.FIT_BATCH, member_rows=rows, permutations=perms)
        for e in range(E):
            if e == poison:
                assert np.all(np.isnan(tl[e])) and np.all(np.isnan(ens.numpy_logvar_head(e)[0]))
                continue
            for a, b in zip(_params(ens, e) + [tl[e], vl[e]], singles[e]):
                np.testing.assert_array_equal(a, b)
        ens.close()


# ---- 4. regularisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
def test_weight_decay_reaches_the_head_kernel_and_not_its_bias(L, mode):
    """weight_decay = [0, 4.0] on 4-16-3: only W_1 and W_v decay; against the float64 rule, which decays W_v with the last
    layer's lambda and b_v never.  (The undecayed fit of the same case differs from it by far more than the tolerance.)"""
    ws, bs, acts, head, tin, tout, vin, vout, perms = N.fit_case(((4, 16, 3), ("tanh", None)), seed=100)
    kw = dict(learning_rate=1e-2, rule="sgd", weight_decay=[0.0, 4.0], decay_mode=mode)
    tr = _trainer(ws, bs, acts, head, **kw)
    losses = tr.fit(tin, tout, vin, vout, N.FIT_EPOCHS, N.FIT_BATCH, permutations=perms)
    want = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, **kw)
    _assert_fit(_params(tr), losses, want)
    plain = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, learning_rate=1e-2, rule="sgd")
    assert np.max(np.abs(plain[2][0] - want[2][0])) > 100 * W_ATOL


def test_weight_decay_on_the_one_layer_net(L):
    """L = 1: the head sits on the input; weight_decay=[4.0] decays W_0 and W_v."""
    ws, bs, acts, head, x, y, idx = N.gradient_case("5-3", 16)
    perms = [np.random.default_rng(5).permutation(128)]
    kw = dict(learning_rate=1e-2, rule="sgd", weight_decay=[4.0], decay_mode="l2")
    tr = _trainer(ws, bs, acts, head, **kw)
    losses = tr.fit(x[:128], y[:128], x[128:], y[128:], 1, 24, permutations=perms)
    want = N.train_nll(ws, bs, acts, head, x[:128], y[:128], x[128:], y[128:], perms, 24, **kw)
    _assert_fit(_params(tr), losses, want)


def test_early_stopping_restores_the_best_head(L):
    c = N.rising_case()
    ws, bs, acts, head, tin, tout, vin, vout, perms = c
    tr = _trainer(ws, bs, acts, head, **N.RISING)
    losses = tr.fit(tin, tout, vin, vout, len(perms), N.FIT_BATCH, permutations=perms)
    want = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, **N.RISING)
    rep = want[5]
    assert (tr.epochs_run, tr.best_epoch) == (rep["epochs_run"], rep["best_epoch"]) == (2, 0)
    np.testing.assert_allclose(tr.best_val, rep["best_val"], rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert np.all(np.isnan(losses[0][2:])) and np.all(np.isnan(losses[1][2:]))
    _assert_fit(_params(tr), losses, want)                                  # the first epoch's parameters, head included
    late = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms[:2], N.FIT_BATCH, rule="sgd", learning_rate=5e-2)
    for a, b in ((late[0][0], want[0][0]), (late[2][1], want[2][1])):       # ... which the second epoch's are not: W_0, b_v
        assert np.max(np.abs(a - b)) > 10 * W_ATOL


# ---- 5. refusals and lifecycle ------------------------------------------------------------------------------------------
def test_refusals_carry_a_code_and_a_message_and_leave_a_usable_trainer(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer, HipGaussianTrainer
    ws, bs, acts, head, tin, tout, vin, vout, perms = N.fit_case("4-16-16-3", seed=110)
    for lo, hi in ((-41.0, 0.5), (-10.0, 40.5), (1.0, 0.5), (float("nan"), 0.5), (-10.0, float("inf"))):
        with pytest.raises(L.BBMPCError) as ei:
            _trainer(ws, bs, acts, (head[0], head[1], lo, hi))
        assert ei.value.code == L.E_INVALID and "min_logvar" in str(ei.value), (lo, hi)
    with pytest.raises(ValueError, match="logvar_head"):                    # a head kernel of the wrong shape
        _trainer(ws, bs, acts, (head[0].T.copy(), head[1], head[2], head[3]))
    with pytest.raises(L.BBMPCError) as ei:
        _ensemble([(ws, bs)] * 9, acts, [head] * 9)
    assert ei.value.code == L.E_UNSUPPORTED and "n_members" in str(ei.value)
    plain = HipDenseTrainer(ws, bs, [CODE[a] for a in acts])
    wv, bv = np.zeros_like(head[0]), np.zeros_like(head[1])
    assert L.lib.bbmpc_trainer_get_logvar_head(plain._t, 0, L.ptr(wv), L.ptr(bv)) == L.E_STATE
    assert "log-variance head" in L.lib.bbmpc_last_error().decode()
    np.testing.assert_array_equal(plain.numpy_params()[0][0], ws[0])        # still a usable trainer
    plain.close()
    tr = _trainer(ws, bs, acts, head, learning_rate=2e-3)
    with pytest.raises(L.BBMPCError) as ei:                                 # fit before data
        tr.fit_resident(1, 16, generator_seed=0)
    assert ei.value.code == L.E_STATE
    tr.set_data(tin, tout, vin, vout)
    with pytest.raises(L.BBMPCError) as ei:
        tr.gradients([0, tin.shape[0]])
    assert ei.value.code == L.E_INVALID
    assert L.lib.bbmpc_trainer_get_logvar_head(tr._t, 1, L.ptr(wv), L.ptr(bv)) == L.E_INVALID
    for got, start in zip(_params(tr), ws + bs + [head[0], head[1]]):
        np.testing.assert_array_equal(got, start)
    losses = tr.fit_resident(N.FIT_EPOCHS, N.FIT_BATCH, permutations=perms)
    want = N.train_nll(ws, bs, acts, head, tin, tout, vin, vout, perms, N.FIT_BATCH, learning_rate=2e-3)
    _assert_fit(_params(tr), losses, want)


def test_create_and_destroy_twenty_gaussian_trainers(L):
    ws, bs, acts, head, x, y, idx = N.gradient_case("4-16-16-3", 16)
    for _ in range(20):
        _trainer(ws, bs, acts, head).close()


# ---- 6. the package -----------------------------------------------------------------------------------------------------
def _box_handler(fn):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    return SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)


def _head_of(m):
    return m.logvar_weights.copy(), m.logvar_bias.copy(), m.min_logvar.copy(), m.max_logvar.copy()


def _rows(obs, acs, mask):
    d_in, d_out = OT.assemble_dataset(obs, acs)
    stats = OT.normalization_stats(d_in[mask], d_out[mask], 3)
    tin, tout = OT.normalize(d_in[mask], d_out[mask], stats, 3)
    vin, vout = OT.normalize(d_in[~mask], d_out[~mask], stats, 3)
    return tin, tout, vin, vout, stats


def test_handler_trains_a_probabilistic_mlp_with_hip_nll(L):
    from blackbox_mpc_amd.dynamics_functions.probabilistic_mlp import ProbabilisticMLP
    from blackbox_mpc_amd.engine import Engine
    obs, acs, rews = _episodes(4, 40, 2, 2)
    acts = ["tanh", "tanh", None]
    fn = ProbabilisticMLP([4, 16, 16, 3], acts, seed=3, min_logvar=[-3.0, -2.5, -2.0], max_logvar=[0.5, 0.25, 0.0])
    h = _box_handler(fn)
    w0, b0, head0 = [w.copy() for w in fn.weights], [b.copy() for b in fn.biases], _head_of(fn)
    d_in, _ = OT.assemble_dataset(obs, acs)
    rng = np.random.default_rng(4)
    mask = rng.random(d_in.shape[0]) > 0.25
    epochs, B = 3, 32
    perms = [rng.permutation(int(mask.sum())) for _ in range(epochs)]
    version = fn._version
    h.train(obs, acs, rews, batch_size=B, learning_rate=2e-3, epochs=epochs, split_mask=mask, permutations=perms, backend="hip_nll")
    tin, tout, vin, vout, stats = _rows(obs, acs, mask)
    want = N.train_nll(w0, b0, acts, head0, tin, tout, vin, vout, perms, B, learning_rate=2e-3)
    _assert_fit(fn.weights + fn.biases + [fn.logvar_weights, fn.logvar_bias], (h.training_loss, h.validation_loss), want)
    assert fn._version > version and not np.array_equal(fn.logvar_weights, head0[0])
    d = vout.astype(np.float64) - U.forward(want[0], want[1], acts, vin)[0][-1]
    np.testing.assert_allclose(h.residual_std(), np.sqrt(np.mean(d * d, axis=0)) * (stats[5] + 1e-7), rtol=1e-4)
    eng = Engine(L.OPT_NONE, L.DYN_MLP, L.REW_PENDULUM, [-2.0], [2.0], dim_s=3, num_agents=1, planning_horizon=2)
    eng.set_mlp(fn.weights, fn.biases, fn.activation_codes)
    eng.set_mlp_logvar_head([fn], fn.min_logvar, fn.max_logvar)             # the engine accepts the fitted head


def test_handler_trains_a_probabilistic_ensemble_in_one_fit(L):
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    obs, acs, rews = _episodes(3, 40, 2, 5)
    acts = ["tanh", "tanh", None]
    fn = EnsembleMLP([4, 16, 16, 3], acts, num_members=3, seed=6, probabilistic=True)
    h = _box_handler(fn)
    start = [([w.copy() for w in m.weights], [b.copy() for b in m.biases], _head_of(m)) for m in fn.members]
    d_in, _ = OT.assemble_dataset(obs, acs)
    rng = np.random.default_rng(7)
    mask = rng.random(d_in.shape[0]) > 0.25
    n, epochs, B = int(mask.sum()), 3, 32
    boots = [rng.integers(0, n, size=n) for _ in range(3)]
    perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(3)]
    versions = [m._version for m in fn.members]
    h.train(obs, acs, rews, batch_size=B, learning_rate=2e-3, epochs=epochs, split_mask=mask, permutations=perms,
            bootstrap_indices=boots, backend="hip_nll")
    tin, tout, vin, vout, stats = _rows(obs, acs, mask)
    sq = []
    for e, m in enumerate(fn.members):
        want = N.train_nll(start[e][0], start[e][1], acts, start[e][2], tin[boots[e]], tout[boots[e]], vin, vout, perms[e], B,
                           learning_rate=2e-3)
        _assert_fit(m.weights + m.biases + [m.logvar_weights, m.logvar_bias], (h.member_training_loss[e], h.member_validation_loss[e]), want)
        assert m._version >= versions[e] + 2                                # set_weights and set_logvar_head
        d = vout.astype(np.float64) - U.forward(want[0], want[1], acts, vin)[0][-1]
        sq.append(np.mean(d * d, axis=0))
    np.testing.assert_array_equal(h.training_loss, h.member_training_loss[0])
    np.testing.assert_allclose(h.residual_std(), np.sqrt(np.mean(sq, axis=0)) * (stats[5] + 1e-7), rtol=1e-4)
    assert not np.allclose(fn.members[0].logvar_weights, fn.members[1].logvar_weights)


def test_hip_nll_on_a_plain_model_gives_the_bits_of_hip(L):
    from blackbox_mpc_amd.dynamics_functions.deterministic_mlp import DeterministicMLP
    obs, acs, rews = _episodes(3, 40, 2, 8)
    d_in, _ = OT.assemble_dataset(obs, acs)
    rng = np.random.default_rng(9)
    mask = rng.random(d_in.shape[0]) > 0.25
    perms = [rng.permutation(int(mask.sum())) for _ in range(2)]
    out = []
    for backend in ("hip", "hip_nll"):
        fn = DeterministicMLP([4, 16, 16, 3], ["tanh", "tanh", None], seed=10)
        h = _box_handler(fn)
        h.train(obs, acs, rews, batch_size=32, learning_rate=2e-3, epochs=2, split_mask=mask, permutations=perms, backend=backend)
        out.append(fn.weights + fn.biases + [h.training_loss, h.validation_loss, h.residual_std()])
    for a, b in zip(*out):
        np.testing.assert_array_equal(a, b)


def test_the_example_runs_in_its_smallest_setting(L):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_hip_probabilistic_ensemble_pendulum.py"), "--small"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "validation NLL" in res.stdout
