"""The hand-written training kernels (csrc/kernels_train.hpp, bbmpc_trainer_*, HipDenseTrainer) on the GPU: gradients
against the float64 oracle with DenseTrainer's own error as the yardstick, whole fits against oracle_train.train at the
tolerances tests/test_gpu_train.py uses for the torch trainer, every activation code, bit reproducibility, refusals and
lifecycle, and the backend="hip" paths of the package."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from oracle import oracle_np as O
from oracle import oracle_train as OT
from tests import train_hip_util as U
from tests.test_gpu_activations import CODE
from tests.test_train_cpu import _episodes, _handler

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


def _trainer(ws, bs, acts, **kw):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer
    return HipDenseTrainer(ws, bs, [CODE[a] for a in acts], None, **kw)


def _assert_fit_matches(tr, losses, want):
    w, b, tl, vl = want
    gw, gb = tr.numpy_params()
    for got, ref in zip(gw + gb, w + b):
        np.testing.assert_allclose(got, ref, rtol=0, atol=W_ATOL)
    np.testing.assert_allclose(losses[0], tl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(losses[1], vl, rtol=LOSS_RTOL, atol=LOSS_ATOL)       # NaN == NaN here


# ---- 1. gradients -----------------------------------------------------------------------------------------------------
NETS = {"4-64-64-3": ((4, 64, 64, 3), ("tanh", "tanh", None)),
        "7-20-33-1": ((7, 20, 33, 1), ("swish", "tanh", None)),
        "46-200-200-1": ((46, 200, 200, 1), ("tanh", "tanh", None))}


def _torch_gradients(ws, bs, codes, x, y):
    """DenseTrainer's gradient of the batch, rebuilt the way DenseTrainer._step does."""
    import torch
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer, _act_grad
    tr = DenseTrainer(ws, bs, codes, "cuda")
    xt, yt = torch.as_tensor(x).to(tr.dev), torch.as_tensor(y).to(tr.dev)
    zs = []
    ys = tr.forward(xt, zs)
    diff = ys[-1] - yt
    g = diff * (2.0 / diff.numel())
    n = len(tr.w)
    gw, gb = [None] * n, [None] * n
    for l in reversed(range(n)):
        g = _act_grad(tr.acts[l], ys[l + 1], g, zs[l])
        gw[l] = ys[l].t() @ g
        gb[l] = g.sum(dim=0)
        if l:
            g = g @ tr.w[l].t()
    return float((diff * diff).mean().item()), [t.cpu().numpy() for t in gw], [t.cpu().numpy() for t in gb]


@pytest.mark.parametrize("B", [16, 24, 40, 128])
@pytest.mark.parametrize("net", sorted(NETS))
def test_gradients_against_the_float64_oracle(L, net, B, capsys):
    dims, acts = NETS[net]
    ws, bs = U.params(dims, seed=11)
    x, y = U.dataset(160, dims[0], dims[-1], seed=12, offset=0.5)         # (why the offset: train_hip_util.dataset)
    idx = np.random.default_rng(13 + B).permutation(160)[:B]
    tr = _trainer(ws, bs, acts)
    tr.set_data(x, y, x[:0], y[:0])
    loss, gw, gb = tr.gradients(idx)
    want_loss, ww, wb = U.mse_and_grads(ws, bs, acts, x[idx], y[idx])
    t_loss, tw, tb = _torch_gradients(ws, bs, [CODE[a] for a in acts], x[idx], y[idx])
    rows = []
    for name, got, tor, want in [("W%d" % l, gw[l], tw[l], ww[l]) for l in range(len(ws))] + \
                                [("b%d" % l, gb[l], tb[l], wb[l]) for l in range(len(ws))]:
        rows.append((name, U.rel_err(got, want), U.rel_err(tor, want)))
    with capsys.disabled():
        print("\n[train_hip] gradient error %s B=%d (max|got-want|/max|want|; hip / torch): %s; loss %.3e / %.3e"
              % (net, B, ", ".join("%s %.2e / %.2e" % r for r in rows), abs(loss - want_loss) / want_loss,
                 abs(t_loss - want_loss) / want_loss))
    for name, e_hip, e_torch in rows:
        assert e_hip <= max(4.0 * e_torch, 1e-6), (name, e_hip, e_torch)
    assert abs(loss - want_loss) <= max(4.0 * abs(t_loss - want_loss), 1e-6 * want_loss)
    np.testing.assert_array_equal(tr.numpy_params()[0][0], ws[0])           # nothing was updated


# ---- 2. whole fits ----------------------------------------------------------------------------------------------------
def _fit_case(dims, acts, n_train, n_val, B, epochs, rule, lr, seed):
    ws, bs = U.params(dims, seed=seed)
    x, y = U.dataset(n_train + n_val, dims[0], dims[-1], seed=seed + 1)
    tin, tout, vin, vout = x[:n_train], y[:n_train], x[n_train:], y[n_train:]
    rng = np.random.default_rng(seed + 2)
    perms = [rng.permutation(n_train) for _ in range(epochs)]
    tr = _trainer(ws, bs, acts, learning_rate=lr, rule=rule)
    losses = tr.fit(tin, tout, vin, vout, epochs, B, permutations=perms)
    want = U.train(ws, bs, list(acts), tin, tout, vin, vout, perms, batch_size=B, learning_rate=lr, rule=rule)
    return tr, losses, want


@pytest.mark.parametrize("rule,lr", [("adam", 2e-3), ("sgd", 1e-2), ("rmsprop", 1e-3)])
def test_fit_matches_the_oracle(L, rule, lr):
    tr, losses, want = _fit_case((4, 64, 64, 3), ("tanh", "tanh", None), 240, 80, 32, 6, rule, lr, seed=20)   # a 75 / 25 split
    _assert_fit_matches(tr, losses, want)
    assert np.all(np.isfinite(losses[1]))


def test_fit_drops_the_remainder_on_odd_widths(L):
    tr, losses, want = _fit_case((7, 20, 33, 1), ("swish", "tanh", None), 100, 50, 24, 5, "adam", 2e-3, seed=30)
    _assert_fit_matches(tr, losses, want)


def test_validation_loss_is_nan_without_a_full_batch(L):
    tr, losses, want = _fit_case((4, 64, 64, 3), ("tanh", "tanh", None), 96, 20, 32, 2, "adam", 2e-3, seed=40)
    assert np.all(np.isnan(want[3])) and np.all(np.isnan(losses[1]))
    _assert_fit_matches(tr, losses, want)


# ---- 3. every activation code -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODE, key=lambda k: CODE[k]))
def test_one_epoch_with_every_activation_code(L, name):
    assert len(CODE) == 13                                                  # `None` + the twelve codes
    tr, losses, want = _fit_case((4, 20, 3), (name, None), 64, 32, 16, 1, "adam", 2e-3, seed=50 + CODE[name])
    _assert_fit_matches(tr, losses, want)


# ---- 4. bits ----------------------------------------------------------------------------------------------------------
def test_equal_fits_give_equal_bits(L):
    dims, acts = (7, 20, 33, 1), ("swish", "tanh", None)
    ws, bs = U.params(dims, seed=60)
    x, y = U.dataset(150, 7, 1, seed=61)
    perms = [np.random.default_rng(62 + e).permutation(100) for e in range(3)]
    runs = []
    for _ in range(2):
        tr = _trainer(ws, bs, acts)
        tl, vl = tr.fit(x[:100], y[:100], x[100:], y[100:], 3, 24, permutations=perms)
        runs.append(tr.numpy_params()[0] + tr.numpy_params()[1] + [tl, vl])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    seeded = []
    for _ in range(2):
        tr = _trainer(ws, bs, acts)
        tl, vl = tr.fit(x[:100], y[:100], x[100:], y[100:], 3, 24, generator_seed=1234)
        seeded.append(tr.numpy_params()[0] + tr.numpy_params()[1] + [tl, vl])
    for a, b in zip(*seeded):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(seeded[0][0], runs[0][0])                     # other permutations, other weights


def test_library_permutations_follow_the_documented_generator(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import draw_permutation
    dims, acts = (4, 20, 3), ("tanh", None)
    ws, bs = U.params(dims, seed=70)
    x, y = U.dataset(90, 4, 3, seed=71)
    perms = [draw_permutation(99, e, 64) for e in range(2)]
    assert sorted(perms[0].tolist()) == list(range(64)) and not np.array_equal(perms[0], perms[1])
    a, b = _trainer(ws, bs, acts), _trainer(ws, bs, acts)
    la = a.fit(x[:64], y[:64], x[64:], y[64:], 2, 16, generator_seed=99)
    lb = b.fit(x[:64], y[:64], x[64:], y[64:], 2, 16, permutations=perms)
    for p, q in zip(a.numpy_params()[0] + list(la), b.numpy_params()[0] + list(lb)):
        np.testing.assert_array_equal(p, q)


# ---- 5. refusals and lifecycle ----------------------------------------------------------------------------------------
def _raw_create(L, dims, acts, ws=None, bs=None, rule=1, lr=1e-3):
    from blackbox_mpc_amd.dynamics_functions._train_hip import _ptr_array
    n = len(dims) - 1
    if ws is None:
        ws = [np.zeros((dims[l], dims[l + 1]), F) for l in range(n)]
        bs = [np.zeros((dims[l + 1],), F) for l in range(n)]
    d, a = np.asarray(dims, np.int32), np.asarray(acts, np.int32)
    i32p = ctypes.POINTER(ctypes.c_int32)
    t = ctypes.c_void_p(None)
    code = L.lib.bbmpc_trainer_create(ctypes.byref(t), -1, n, d.ctypes.data_as(i32p), a.ctypes.data_as(i32p), _ptr_array(ws),
                                      _ptr_array(bs), rule, lr)
    return code, t, L.lib.bbmpc_last_error().decode()


def test_refusals_carry_a_code_and_a_message(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import lds_bytes_formula
    for dims, acts, kw, want in [((4,) + (8,) * 8 + (3,), (1,) * 9, {}, L.E_UNSUPPORTED),          # nine layers
                                 ((4, 513, 3), (1, 0), {}, L.E_UNSUPPORTED),                      # a width over 512
                                 ((4, 0, 3), (1, 0), {}, L.E_INVALID),
                                 ((4, 8, 3), (13, 0), {}, L.E_INVALID),                           # unknown activation
                                 ((4, 8, 3), (1, 0), {"rule": 7}, L.E_INVALID),
                                 ((4, 8, 3), (1, 0), {"lr": float("nan")}, L.E_INVALID)]:
        code, t, msg = _raw_create(L, dims, acts, **kw)
        assert code == want and not t.value and "trainer" in msg, (dims, code, msg)
    # the 8 x 512 network: accepted or refused exactly as the documented formula says
    dims, acts = (512,) * 9, (1,) * 8
    fits = lds_bytes_formula(dims, acts) <= L.TRAIN_LDS_LIMIT
    code, t, msg = _raw_create(L, dims, acts)
    assert (code == 0) == fits and (fits or (code == L.E_UNSUPPORTED and "LDS" in msg))
    L.lib.bbmpc_trainer_destroy(t)
    # the widest network the other shapes of profiles/train_hip.md need is accepted
    code, t, _ = _raw_create(L, (26, 500, 500, 500, 20), (1, 1, 1, 0))
    assert code == 0 and lds_bytes_formula((26, 500, 500, 500, 20), (1, 1, 1, 0)) <= L.TRAIN_LDS_LIMIT
    L.lib.bbmpc_trainer_destroy(t)
    assert L.lib.bbmpc_trainer_destroy(None) == 0
    assert L.lib.bbmpc_trainer_fit(None, 1, 16, None, 0, None, None) == L.E_INVALID


def test_a_refused_call_leaves_a_usable_trainer(L):
    dims, acts = (4, 20, 3), ("tanh", None)
    ws, bs = U.params(dims, seed=80)
    x, y = U.dataset(80, 4, 3, seed=81)
    tr = _trainer(ws, bs, acts)
    for got, want in zip(sum(tr.numpy_params(), []), ws + bs):             # before any fit: the initial weights, bit for bit
        np.testing.assert_array_equal(got, want)
    with pytest.raises(L.BBMPCError) as ei:                                 # fit before data
        tr.fit_resident(1, 16, permutations=None, generator_seed=0)
    assert ei.value.code == L.E_STATE
    tr.set_data(x[:64], y[:64], x[64:], y[64:])
    for B in (0, 4097):
        with pytest.raises(L.BBMPCError) as ei:
            tr.fit_resident(1, B, generator_seed=0)
        assert ei.value.code == L.E_UNSUPPORTED and "batch_size" in str(ei.value)
    with pytest.raises(L.BBMPCError) as ei:
        tr.fit_resident(1, 16, permutations=[np.arange(64) + 1])           # an entry outside the rows
    assert ei.value.code == L.E_INVALID
    with pytest.raises(L.BBMPCError) as ei:
        tr.gradients([0, 64])
    assert ei.value.code == L.E_INVALID
    for got, want in zip(sum(tr.numpy_params(), []), ws + bs):
        np.testing.assert_array_equal(got, want)
    perms = [np.random.default_rng(82).permutation(64)]
    losses = tr.fit_resident(1, 16, permutations=perms)
    want = U.train(ws, bs, list(acts), x[:64], y[:64], x[64:], y[64:], perms, batch_size=16, learning_rate=1e-3)
    _assert_fit_matches(tr, losses, want)
    d = y[64:].astype(np.float64) - U.forward(want[0], want[1], acts, x[64:])[0][-1]
    np.testing.assert_allclose(tr.residual_rms(x[64:], y[64:]), np.sqrt(np.mean(d * d, axis=0)), rtol=1e-4, atol=1e-6)
    assert tr.residual_rms(x[:0], y[:0]) is None


def test_create_and_destroy_fifty_trainers(L):
    ws, bs = U.params((4, 20, 3), seed=90)
    for _ in range(50):
        _trainer(ws, bs, ("tanh", None)).close()


# ---- 6. the package's backend="hip" paths -------------------------------------------------------------------------------
def test_handler_train_with_the_hip_backend_and_the_engine_picks_the_weights_up(L):
    from blackbox_mpc_amd.trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    obs, acs, rews = _episodes(4, 40, 2, 2)
    h, fn = _handler(layers=(4, 64, 64, 3), acts=("tanh", "tanh", None), seed=3)
    w0, b0 = [w.copy() for w in fn.weights], [b.copy() for b in fn.biases]
    ev = DeterministicTrajectoryEvaluator(pendulum_reward_function, h)
    s = O.pendulum_start_states(2)
    a = np.random.default_rng(1).uniform(-2, 2, (2, 1)).astype(F)
    h.set_normalization_stats(np.zeros(3), np.ones(3), np.zeros(1), np.ones(1), np.zeros(3), np.ones(3))   # placeholders: the
    before = ev.predict_next_state(s, a)                # first train() computes the real ones; the engine holds the untrained weights now
    d_in, d_out = OT.assemble_dataset(obs, acs)
    rng = np.random.default_rng(4)
    mask = rng.random(d_in.shape[0]) > 0.25
    epochs, B = 6, 32
    perms = [rng.permutation(int(mask.sum())) for _ in range(epochs)]
    h.train(obs, acs, rews, batch_size=B, learning_rate=2e-3, epochs=epochs, split_mask=mask, permutations=perms, backend="hip")
    stats = OT.normalization_stats(d_in[mask], d_out[mask], 3)
    tin, tout = OT.normalize(d_in[mask], d_out[mask], stats, 3)
    vin, vout = OT.normalize(d_in[~mask], d_out[~mask], stats, 3)
    w, b, tl, vl = OT.train(w0, b0, ["tanh", "tanh", None], tin, tout, vin, vout, perms, batch_size=B, learning_rate=2e-3)
    for got, want in zip(fn.weights + fn.biases, w + b):
        np.testing.assert_allclose(got, want, rtol=0, atol=W_ATOL)
    np.testing.assert_allclose(h.training_loss, tl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(h.validation_loss, vl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert h.residual_std().shape == (3,)
    x, _ = OT.normalize(np.concatenate([s, a], 1), np.zeros((2, 3), F), h.normalization_stats(), 3)
    raw = OT.forward(fn.weights, fn.biases, ["tanh", "tanh", None], x)[-1]
    ms, ss, ma, sa_, mt, st = h.normalization_stats()
    after = ev.predict_next_state(s, a)
    np.testing.assert_allclose(after, s + mt + raw * (st + 1e-7), rtol=2e-5, atol=2e-5)
    assert not np.allclose(after, before)


def test_ensemble_members_with_the_hip_backend(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    obs, acs, rews = _episodes(3, 40, 2, 5)
    acts = ["tanh", "tanh", None]
    fn = EnsembleMLP([4, 32, 32, 3], acts, num_members=2, seed=6)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)
    start = [([w.copy() for w in m.weights], [b.copy() for b in m.biases]) for m in fn.members]
    d_in, d_out = OT.assemble_dataset(obs, acs)
    rng = np.random.default_rng(7)
    mask = rng.random(d_in.shape[0]) > 0.25
    n, epochs, B = int(mask.sum()), 3, 32
    boots = [rng.integers(0, n, size=n) for _ in range(2)]
    perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(2)]
    h.train(obs, acs, rews, batch_size=B, learning_rate=2e-3, epochs=epochs, split_mask=mask, permutations=perms,
            bootstrap_indices=boots, backend="hip")
    stats = OT.normalization_stats(d_in[mask], d_out[mask], 3)
    tin, tout = OT.normalize(d_in[mask], d_out[mask], stats, 3)
    vin, vout = OT.normalize(d_in[~mask], d_out[~mask], stats, 3)
    for e, member in enumerate(fn.members):
        w, b, tl, vl = OT.train(start[e][0], start[e][1], acts, tin[boots[e]], tout[boots[e]], vin, vout, perms[e], batch_size=B,
                                learning_rate=2e-3)
        for got, want in zip(member.weights + member.biases, w + b):
            np.testing.assert_allclose(got, want, rtol=0, atol=W_ATOL)
        np.testing.assert_allclose(h.member_training_loss[e], tl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
        np.testing.assert_allclose(h.member_validation_loss[e], vl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    assert not np.allclose(fn.members[0].weights[0], fn.members[1].weights[0])


def _check_model_fit(model, x_raw, y_raw, w0, b0, acts, seed, epochs, B, losses):
    """A reward / value / policy model's train(backend="hip", seed=...) against oracle_train.train on its normalised rows,
    split and permutations restated from the seed."""
    from blackbox_mpc_amd.dynamics_functions._train_hip import draw_permutation
    stats = model.normalization_stats()
    xn = (x_raw - stats[0]) / (stats[1] + F(1e-7))
    yn = (y_raw - stats[2]) / stats[3]
    order = np.random.default_rng(seed).permutation(x_raw.shape[0])
    n_val = int(x_raw.shape[0] * 0.2)
    val, trn = order[:n_val], order[n_val:]
    perms = [draw_permutation(seed, e, len(trn)) for e in range(epochs)]
    w, b, tl, vl = OT.train(w0, b0, acts, xn[trn], yn[trn], xn[val], yn[val], perms, batch_size=B, learning_rate=2e-3)
    for got, want in zip(model.weights + model.biases, w + b):
        np.testing.assert_allclose(got, want, rtol=0, atol=W_ATOL)
    np.testing.assert_allclose(losses[0], tl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(losses[1], vl, rtol=LOSS_RTOL, atol=LOSS_ATOL)


def test_reward_value_and_policy_models_with_the_hip_backend(L):
    from blackbox_mpc_amd.policy_functions.learned_policy_mlp import LearnedPolicyMLP
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    from blackbox_mpc_amd.value_functions.learned_value_mlp import LearnedValueMLP
    rng = np.random.default_rng(100)
    n, S, Ud, epochs, B, seed = 200, 3, 1, 3, 32, 5
    s, a, s2 = rng.normal(size=(n, S)).astype(F), rng.uniform(-2, 2, (n, Ud)).astype(F), rng.normal(size=(n, S)).astype(F)
    r = (-(s[:, 0] ** 2) - 0.1 * a[:, 0] ** 2 + 0.3 * s2[:, 1]).astype(F)
    kw = dict(epochs=epochs, batch_size=B, learning_rate=2e-3, validation_split=0.2, seed=seed, backend="hip")
    acts = ["tanh", "tanh", None]
    rew = LearnedRewardMLP(S, Ud, [32, 32, 1], acts, seed=1)
    w0, b0 = [w.copy() for w in rew.weights], [b.copy() for b in rew.biases]
    losses = rew.train(s, a, s2, r, **kw)
    _check_model_fit(rew, rew.assemble_inputs(s, a, s2).astype(F), r.reshape(-1, 1), w0, b0, acts, seed, epochs, B, losses)
    val = LearnedValueMLP(S, [32, 32, 1], acts, seed=2)
    w0, b0 = [w.copy() for w in val.weights], [b.copy() for b in val.biases]
    losses = val.train(s, r, **kw)
    _check_model_fit(val, s, r.reshape(-1, 1), w0, b0, acts, seed, epochs, B, losses)
    pol = LearnedPolicyMLP(S, Ud, [32, 32, Ud], acts, seed=3)
    w0, b0 = [w.copy() for w in pol.weights], [b.copy() for b in pol.biases]
    losses = pol.train(s, a, **kw)
    _check_model_fit(pol, s, a, w0, b0, acts, seed, epochs, B, losses)


def test_the_example_runs_in_its_smallest_setting(L):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_hip_pendulum.py"), "--small"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "validation loss" in res.stdout


# ---- 7. rate print ----------------------------------------------------------------------------------------------------
def test_training_step_rate_of_both_trainers(L, capsys):
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    rng = np.random.default_rng(0)
    n = 32768
    din, dout = rng.normal(size=(n, 26)).astype(F), rng.normal(size=(n, 20)).astype(F)
    ws, bs = O.make_mlp_params([26, 200, 200, 20], seed=1)
    rates = {}
    for name in ("torch", "hip"):
        tr = DenseTrainer(ws, bs, [1, 1, 0], "cuda") if name == "torch" else _trainer(ws, bs, ("tanh", "tanh", None))
        tr.fit(din, dout, din[:256], dout[:256], 1, 128, generator_seed=0)
        t0 = time.perf_counter()
        tl, _ = tr.fit(din, dout, din[:256], dout[:256], 2, 128, generator_seed=1)
        rates[name] = 2 * (n // 128) / (time.perf_counter() - t0)
        assert np.all(np.isfinite(tl))
    with capsys.disabled():
        print("\n[train_hip] Adam steps/s (26-200-200-20, batch 128, whole fit incl. upload): DenseTrainer (graph) %.0f, "
              "HipDenseTrainer %.0f" % (rates["torch"], rates["hip"]))
