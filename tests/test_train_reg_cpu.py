"""Weight decay, early stopping and best-weights restore on the host: DenseTrainer(device="cpu")
against the float64 statement of the rule (tests/train_reg_util.py), the monitor's state machine on injected losses, how the
training surfaces hand the options on, the refusals that come before the library is called, and the three new entry points
of the C ABI.

Tolerances are tests/test_train_cpu.py's for the same comparison (float32 torch against the float64 oracle): weights 2e-4
absolute under adam and 3e-4 under sgd / rmsprop, losses 1e-4 / 2e-4 relative.  The decay adds one multiply-add per weight
and step to a chain of that length, which those bounds already cover."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import train_hip_util as U
from tests import train_reg_util as RU
from tests.test_gpu_activations import CODE
from tests.test_train_cpu import _episodes, _handler

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W_ATOL = {"adam": 2e-4, "sgd": 3e-4, "rmsprop": 3e-4}
LOSS_RTOL = {"adam": 1e-4, "sgd": 2e-4, "rmsprop": 2e-4}
NETS = {"4-8-3": ((4, 8, 3), ("tanh", None), 16), "17-33-5": ((17, 33, 5), ("tanh", None), 17)}
REG_SYMBOLS = ("bbmpc_trainer_set_weight_decay", "bbmpc_trainer_set_early_stopping", "bbmpc_trainer_get_fit_report")
OPTIONS = ("weight_decay", "decay_mode", "patience", "min_delta", "restore_best")


def _case(net, seed=5, rows=3):
    dims, acts, B = NETS[net]
    ws, bs = U.params(dims, seed)
    x, y = U.dataset((rows + 1) * B + 3, dims[0], dims[-1], seed + 1)
    n = rows * B + 3                                                # a dropped remainder; one full validation batch
    return dims, acts, B, ws, bs, x[:n], y[:n], x[n:], y[n:]


def _torch_trainer(ws, bs, acts, **kw):
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    return DenseTrainer(ws, bs, [CODE[a] for a in acts], "cpu", **kw)


@pytest.mark.parametrize("rule", ["adam", "sgd", "rmsprop"])
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("net", sorted(NETS))
def test_the_torch_trainer_follows_the_float64_statement(net, mode, rule):
    dims, acts, B, ws, bs, tx, ty, vx, vy = _case(net)
    epochs, lr, decay = 6, 2e-2, [0.5, 0.25]
    perms = [np.random.default_rng(40 + k).permutation(tx.shape[0]) for k in range(epochs)]
    tr = _torch_trainer(ws, bs, acts, learning_rate=lr, rule=rule, weight_decay=decay, decay_mode=mode)
    tl, vl = tr.fit(tx, ty, vx, vy, epochs, B, permutations=perms)
    w, b, wtl, wvl, rep = RU.train(ws, bs, acts, tx, ty, vx, vy, perms, B, lr, rule, weight_decay=decay, decay_mode=mode)
    gw, gb = tr.numpy_params()
    for got, want in zip(gw + gb, w + b):
        np.testing.assert_allclose(got, want, rtol=0, atol=W_ATOL[rule])
    np.testing.assert_allclose(tl, wtl, rtol=LOSS_RTOL[rule], atol=1e-6)
    np.testing.assert_allclose(vl, wvl, rtol=LOSS_RTOL[rule], atol=1e-6)
    assert (tr.epochs_run, tr.best_epoch) == (epochs, -1) and np.isnan(tr.best_val)
    # the case tells the modes from each other and from no decay: the statements lie fifty tolerances apart
    plain = RU.train(ws, bs, acts, tx, ty, vx, vy, perms, B, lr, rule)[0]
    other = RU.train(ws, bs, acts, tx, ty, vx, vy, perms, B, lr, rule, weight_decay=decay,
                     decay_mode="l2" if mode == "decoupled" else "decoupled")[0]
    for l in range(2):
        assert np.max(np.abs(plain[l] - w[l])) > 50 * W_ATOL[rule]
    if rule != "sgd":                                               # under plain SGD the two modes are the same rule
        assert max(np.max(np.abs(o - x)) for o, x in zip(other, w)) > 10 * W_ATOL[rule]


@pytest.mark.parametrize("rule", ["adam", "sgd", "rmsprop"])
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
def test_a_zero_data_gradient_leaves_the_biases_bit_equal(mode, rule):
    dims, acts, B, ws, bs, tx, ty, vx, vy = _case("17-33-5")
    ws[-1][:], bs[-1][:] = 0.0, 0.0                                 # f(x) = 0 = the targets: every data gradient is exactly 0
    ty, vy = np.zeros_like(ty), np.zeros_like(vy)
    perms = [np.arange(tx.shape[0])] * 3
    out = {}
    for decay in (0.0, [0.5, 0.25]):
        tr = _torch_trainer(ws, bs, acts, learning_rate=2e-2, rule=rule, weight_decay=decay, decay_mode=mode)
        losses = tr.fit(tx, ty, vx, vy, 3, B, permutations=perms)
        assert np.all(losses[0] == 0.0)
        out[np.ndim(decay)] = tr.numpy_params()
    for plain, decayed, start in zip(out[0][1], out[1][1], bs):
        np.testing.assert_array_equal(decayed, plain)
        np.testing.assert_array_equal(decayed, start)
    np.testing.assert_array_equal(out[0][0][0], ws[0])              # nothing moves without decay
    assert np.mean(out[1][0][0] != ws[0]) > 0.99                    # and the first kernel moves with it
    np.testing.assert_array_equal(out[1][0][1], ws[1])              # a zero kernel stays zero


def test_the_monitor_on_an_injected_loss_sequence():
    from blackbox_mpc_amd.dynamics_functions._train_reg import Monitor
    nan = float("nan")

    def run(vals, patience, min_delta):
        mon, flags = Monitor(patience, min_delta), []
        for k, v in enumerate(vals):
            improved, stop = mon.update(k, v)
            flags.append(improved)
            if stop:
                break
        got = (len(flags), mon.best_epoch, mon.best_val, flags)
        want = RU.monitor_sequence(vals, patience, min_delta)
        assert got[:2] == want[:2] and got[3] == want[3]
        np.testing.assert_equal(np.float32(got[2]), np.float32(want[2]))
        return got

    # improvement, improvement, a tie within min_delta, NaN, worse: patience 3 is hit at epoch 4
    ran, best, val, flags = run([1.0, 0.5, 0.4995, nan, 0.6, 0.1, 0.05], 3, 1e-3)
    assert (ran, best, flags) == (5, 1, [True, True, False, False, False]) and val == 0.5
    # the same losses with patience 4: epoch 5 improves in time and resets the wait
    ran, best, val, flags = run([1.0, 0.5, 0.4995, nan, 0.6, 0.1, 0.05], 4, 1e-3)
    assert (ran, best, flags[5:]) == (7, 6, [True, True])
    # patience 0 never stops; an equal loss is no improvement at min_delta 0
    ran, best, val, flags = run([2.0, 2.0, 3.0, 1.0], 0, 0.0)
    assert (ran, best, flags) == (4, 3, [True, False, False, True])
    # nothing but NaN: no best epoch, and the wait runs into the patience
    ran, best, val, flags = run([nan] * 6, 2, 0.0)
    assert (ran, best) == (2, -1) and np.isnan(val) and not any(flags)
    # a huge min_delta: only the first finite loss improves (on +inf)
    ran, best, val, flags = run([5.0, 4.0, 3.0, 2.0, 1.0, 0.5], 2, 1e9)
    assert (ran, best, val) == (3, 0, 5.0)


def test_the_torch_trainer_stops_restores_and_reports():
    dims, acts, B, ws, bs, tx, ty, vx, vy = _case("4-8-3")
    perms = [np.random.default_rng(60 + k).permutation(tx.shape[0]) for k in range(6)]
    kw = dict(learning_rate=2e-2, rule="adam")
    tr = _torch_trainer(ws, bs, acts, patience=2, min_delta=1e9, **kw)
    tl, vl = tr.fit(tx, ty, vx, vy, 6, B, permutations=perms)
    assert (tr.epochs_run, tr.best_epoch) == (3, 0) and tr.best_val == vl[0]
    assert np.all(np.isfinite(tl[:3])) and np.all(np.isnan(tl[3:])) and np.all(np.isnan(vl[3:]))
    free3 = _torch_trainer(ws, bs, acts, **kw)
    free3.fit(tx, ty, vx, vy, 3, B, permutations=perms)
    for got, want in zip(sum(tr.numpy_params(), []), sum(free3.numpy_params(), [])):
        np.testing.assert_array_equal(got, want)
    rs = _torch_trainer(ws, bs, acts, patience=2, min_delta=1e9, restore_best=True, **kw)
    rs.fit(tx, ty, vx, vy, 6, B, permutations=perms)
    free1 = _torch_trainer(ws, bs, acts, **kw)
    free1.fit(tx, ty, vx, vy, 1, B, permutations=perms)
    for got, want in zip(sum(rs.numpy_params(), []), sum(free1.numpy_params(), [])):
        np.testing.assert_array_equal(got, want)
    # the float64 statement reports the same fit
    rep = RU.train(ws, bs, acts, tx, ty, vx, vy, perms, B, 2e-2, "adam", patience=2, min_delta=1e9, restore_best=True)[4]
    assert (rep["epochs_run"], rep["best_epoch"]) == (3, 0)


def test_a_log_variance_head_is_decayed_and_monitored_on_the_nll():
    dims, acts, B, ws, bs, tx, ty, vx, vy = _case("4-8-3")
    rng = np.random.default_rng(3)
    head = (rng.normal(0, 0.3, size=(8, 3)).astype(F), np.zeros((3,), F), -10.0, 0.5)
    tx, ty = tx[:B], ty[:B]                                         # one batch per epoch
    perms = [np.arange(B)] * 2
    tr = _torch_trainer(ws, bs, acts, learning_rate=1e-3, rule="sgd", logvar_head=head, weight_decay=[0.0, 4.0], restore_best=True)
    tl, vl = tr.fit(tx, ty, vx, vy, 2, B, permutations=perms)
    plain = _torch_trainer(ws, bs, acts, learning_rate=1e-3, rule="sgd", logvar_head=head)
    ptl, pvl = plain.fit(tx, ty, vx, vy, 2, B, permutations=perms)
    assert tl[0] == ptl[0] and vl[0] != pvl[0]                      # the reported loss is the data term (the NLL before any step)
    assert tr.best_epoch in (0, 1) and tr.best_val == vl[tr.best_epoch]
    assert np.max(np.abs(tr.numpy_logvar_head()[0] - plain.numpy_logvar_head()[0])) > 1e-3      # W_v saw the last layer's lambda


class _FakeTrainer:
    """Today's DenseTrainer surface: anything new in the call is a TypeError."""
    has_logvar_head = False
    calls = []

    def __init__(self, weights, biases, act_codes, device, learning_rate=1e-3, rule="adam", logvar_head=None, **extra):
        self.w, self.b, self.extra = [np.array(w) for w in weights], [np.array(b) for b in biases], extra
        _FakeTrainer.calls.append(extra)
        self.epochs_run, self.best_epoch = 2, 1

    def fit(self, train_in, train_out, val_in, val_out, epochs, batch_size, permutations=None, generator_seed=None):
        return np.zeros((epochs,)), np.zeros((epochs,))

    def residual_rms(self, val_in, val_out):
        return None

    def numpy_params(self):
        return self.w, self.b


def _fake_dense_trainer(backend, weights, biases, act_codes, device, **kwargs):
    return _FakeTrainer(weights, biases, act_codes, device, **kwargs)


def test_the_training_surfaces_forward_the_options_and_nothing_at_defaults(built_lib, monkeypatch):
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.policy_functions.learned_policy_mlp import LearnedPolicyMLP
    from blackbox_mpc_amd.reward_functions.learned_reward_mlp import LearnedRewardMLP
    from blackbox_mpc_amd.value_functions.learned_value_mlp import LearnedValueMLP
    monkeypatch.setattr(T, "dense_trainer", _fake_dense_trainer)
    obs, acs, rews = _episodes(1, 20, 2, 0)
    s, a, n, r = obs[0][:-1, 0], acs[0][:, 0], obs[0][1:, 0], rews[0][:, 0]
    opts = dict(weight_decay=[1e-4, 2e-4], decay_mode="decoupled", patience=3, min_delta=1e-3, restore_best=True)

    def surfaces():
        h, _ = _handler(layers=(4, 8, 3), acts=("tanh", None))
        yield "handler", lambda **kw: h.train(obs, acs, rews, epochs=2, batch_size=8, device="cpu", seed=0, **kw), h
        he, _ = _handler(layers=(4, 8, 3), acts=("tanh", None))
        he._dynamics_function = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=0)
        yield "ensemble", lambda **kw: he.train(obs, acs, rews, epochs=2, batch_size=8, device="cpu", seed=0, **kw), he
        rm = LearnedRewardMLP(3, 1, [8, 1], ["tanh", None], seed=0)
        yield "reward", lambda **kw: rm.train(s, a, n, r, epochs=2, batch_size=8, device="cpu", seed=0, **kw), rm
        vm = LearnedValueMLP(3, [8, 1], ["tanh", None], seed=0)
        yield "value", lambda **kw: vm.train(s, r, epochs=2, batch_size=8, device="cpu", seed=0, **kw), vm
        yield "value rollouts", lambda **kw: vm.train_on_rollouts(obs, rews, 3, epochs=2, batch_size=8, device="cpu", seed=0, **kw), vm
        pm = LearnedPolicyMLP(3, 1, [8, 1], ["tanh", None], seed=0)
        yield "policy", lambda **kw: pm.train(s, a, epochs=2, batch_size=8, device="cpu", seed=0, **kw), pm
        yield "policy rollouts", lambda **kw: pm.train_on_rollouts(obs, acs, epochs=2, batch_size=8, device="cpu", seed=0, **kw), pm

    for name, call, owner in surfaces():
        _FakeTrainer.calls = []
        call()
        assert _FakeTrainer.calls and all(extra == {} for extra in _FakeTrainer.calls), name
        _FakeTrainer.calls = []
        call(**opts)
        assert _FakeTrainer.calls and all(extra == opts for extra in _FakeTrainer.calls), name
        assert (owner.epochs_run, owner.best_epoch) == (2, 1), name
        _FakeTrainer.calls = []
        call(patience=2)                                            # one option alone travels alone
        assert all(extra == {"patience": 2} for extra in _FakeTrainer.calls), name
        if name == "ensemble":
            assert owner.member_epochs_run == [2, 2] and owner.member_best_epoch == [1, 1]
    with pytest.raises(TypeError):                                  # keyword-only
        LearnedValueMLP(3, [8, 1], ["tanh", None], seed=0).train(s, r, 2, 8, 1e-3, 0.2, "cpu", 0, True, "torch", 1e-4)


def test_the_learning_utilities_hand_the_options_through(built_lib, monkeypatch):
    import inspect
    from blackbox_mpc_amd.utils import dynamics_learning
    src = inspect.getsource(dynamics_learning.learn_dynamics_from_policy)
    for args in ("**train_args)", "reward_train_args or {}", "value_train_args or {}", "policy_train_args or {}"):
        assert args in src
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    params = inspect.signature(SystemDynamicsHandler.train).parameters
    for name in OPTIONS:
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY


def test_monitoring_without_a_validation_batch_is_refused():
    dims, acts, B, ws, bs, tx, ty, vx, vy = _case("4-8-3")
    for kw in (dict(patience=1), dict(restore_best=True)):
        tr = _torch_trainer(ws, bs, acts, **kw)
        with pytest.raises(ValueError, match="validation"):
            tr.fit(tx, ty, vx[:B - 1], vy[:B - 1], 2, B, permutations=[np.arange(tx.shape[0])] * 2)
        for got, want in zip(sum(tr.numpy_params(), []), ws + bs):
            np.testing.assert_array_equal(got, want)                # before anything ran
    obs, acs, rews = _episodes(1, 20, 2, 0)
    h, fn = _handler(layers=(4, 8, 3), acts=("tanh", None))
    with pytest.raises(ValueError, match="validation"):
        h.train(obs, acs, rews, epochs=2, batch_size=8, device="cpu", seed=0, split_mask=np.ones(40, bool), patience=1)


def test_the_entry_points_are_declared_and_bound(built_lib):
    from blackbox_mpc_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text)             # entry points added, no struct changed
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in REG_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(L.lib, name).argtypes is not None, name
    for mode, value in (("L2", L.TRAIN_DECAY_L2), ("DECOUPLED", L.TRAIN_DECAY_DECOUPLED)):
        assert re.search(r"#define\s+BBMPC_TRAIN_DECAY_%s\s+%d\b" % (mode, value), text)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError("the library was called: %s" % name)


def test_bad_options_are_value_errors_before_the_library_is_called(built_lib, monkeypatch):
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer, HipEnsembleTrainer
    ws, bs = U.params((4, 8, 3), seed=0)
    monkeypatch.setattr(L, "lib", _NoLibrary())
    bad = [dict(weight_decay=-1e-3), dict(weight_decay=[1e-3, -1e-3]), dict(weight_decay=float("nan")), dict(weight_decay=[1e-3]),
           dict(decay_mode="l1"), dict(patience=-1), dict(min_delta=-1.0), dict(min_delta=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            HipDenseTrainer(ws, bs, [1, 0], **kw)
        with pytest.raises(ValueError):
            HipEnsembleTrainer([ws, ws], [bs, bs], [1, 0], **kw)
        with pytest.raises(ValueError):
            _torch_trainer(ws, bs, ("tanh", None), **kw)
    obs, acs, rews = _episodes(1, 10, 2, 0)
    h, fn = _handler(layers=(4, 8, 3), acts=("tanh", None))
    for kw in (dict(weight_decay=-1.0), dict(decay_mode="l1"), dict(patience=-1)):
        with pytest.raises(ValueError):
            h.train(obs, acs, rews, epochs=1, batch_size=8, backend="hip", **kw)
    assert h._model_training_in.shape[0] == 0                       # refused before the dataset grew
