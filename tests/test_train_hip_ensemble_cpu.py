"""The one-launch ensemble trainer without a GPU: the C ABI declares, exports and binds its entry points, every refusal that
is argument checking comes before any device, the member seed rule, and what `SystemDynamicsHandler._train_ensemble` hands
to `HipEnsembleTrainer` (a recording fake stands in for it) and does with what it returns."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.test_train_cpu import _episodes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ENSEMBLE_SYMBOLS = ["bbmpc_trainer_create_ensemble", "bbmpc_trainer_set_member_rows", "bbmpc_trainer_fit_ensemble",
                    "bbmpc_trainer_get_member_params", "bbmpc_trainer_residual_rms_ensemble"]


def test_the_ensemble_entry_points_are_declared_and_bound(built_lib):
    from blackbox_mpc_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "bbmpc.h")).read()
    assert re.search(r"#define\s+BBMPC_ABI_VERSION\s+4\b", text) and L.ABI_VERSION == 4      # entry points added, no struct changed
    assert L.lib.bbmpc_abi_version() == 4
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(built_lib)
    for name in ENSEMBLE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in L.SYMBOLS and hasattr(lib, name)
        assert getattr(L.lib, name).argtypes is not None, name
    assert len(L.lib.bbmpc_trainer_create_ensemble.argtypes) == 10 and len(L.lib.bbmpc_trainer_fit_ensemble.argtypes) == 7


def _zeros(dims, E):
    ws = [[np.zeros((i, o), F) for i, o in zip(dims[:-1], dims[1:])] for _ in range(E)]
    bs = [[np.zeros((o,), F) for o in dims[1:]] for _ in range(E)]
    return ws, bs


def test_refusals_come_before_any_device(built_lib):
    from blackbox_mpc_amd import _lib as L
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    for dims, acts, E, code in [((4, 8, 3), [1, 0], 0, L.E_UNSUPPORTED), ((4, 8, 3), [1, 0], 9, L.E_UNSUPPORTED),
                                ((4,) + (8,) * 8 + (3,), [1] * 9, 2, L.E_UNSUPPORTED),           # nine layers
                                ((4, 513, 3), [1, 0], 2, L.E_UNSUPPORTED),                       # a width over 512
                                ((512,) * 9, [1] * 8, 2, L.E_UNSUPPORTED),                       # the LDS carve
                                ((4, 8, 3), [13, 0], 2, L.E_INVALID)]:
        ws, bs = _zeros(dims, E)
        with pytest.raises(L.BBMPCError) as ei:
            T.HipEnsembleTrainer(ws, bs, acts)
        assert ei.value.code == code and "trainer" in str(ei.value), (dims, E, str(ei.value))
    # a NULL handle, on every entry point that takes one
    vp = ctypes.c_void_p
    for call in (lambda: L.lib.bbmpc_trainer_set_member_rows(None, None),
                 lambda: L.lib.bbmpc_trainer_fit_ensemble(None, 1, 16, None, 0, None, None),
                 lambda: L.lib.bbmpc_trainer_get_member_params(None, 0, (vp * 1)(), (vp * 1)()),
                 lambda: L.lib.bbmpc_trainer_residual_rms_ensemble(None, None, None, 1, None)):
        assert call() == L.E_INVALID and "trainer" in L.lib.bbmpc_last_error().decode()
    out = vp(None)
    i32p = ctypes.POINTER(ctypes.c_int32)
    d, a = np.asarray([4, 8, 3], np.int32), np.asarray([1, 0], np.int32)
    assert L.lib.bbmpc_trainer_create_ensemble(ctypes.byref(out), -1, 2, 2, d.ctypes.data_as(i32p), a.ctypes.data_as(i32p), None, None,
                                               1, 1e-3) == L.E_INVALID
    assert "trainer" in L.lib.bbmpc_last_error().decode() and not out.value
    assert L.lib.bbmpc_trainer_create_ensemble(None, -1, 2, 2, d.ctypes.data_as(i32p), a.ctypes.data_as(i32p), None, None, 1,
                                               1e-3) == L.E_INVALID
    # the 2^31 bound on the composed index array [E][epochs][n], as the wrapper restates it before the call
    for E, epochs, n in ((8, 1 << 20, 256), (1, 1 << 16, 1 << 15), (5, 429497, 1000)):
        with pytest.raises(L.BBMPCError) as ei:
            T.check_index_bound(E, epochs, n)
        assert ei.value.code == L.E_UNSUPPORTED and "trainer" in str(ei.value)
    T.check_index_bound(8, (1 << 20) - 1, 256)
    T.check_index_bound(5, 429496, 1000)


def test_the_member_seed_rule():
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipEnsembleTrainer, member_seed
    mask = (1 << 64) - 1
    for seed in (0, 7, 0xFEDCBA9876543210, mask):
        seeds = [member_seed(seed, e) for e in range(8)]
        assert seeds[0] == seed and len(set(seeds)) == 8 and all(0 <= s <= mask for s in seeds)
        for e in range(8):
            assert seeds[e] == seed ^ ((0x9E3779B97F4A7C15 * e) % (1 << 64))
    assert 0x9E3779B97F4A7C15 * 2 > mask and member_seed(0, 2) == (0x9E3779B97F4A7C15 * 2) - (1 << 64)     # wraps
    assert HipEnsembleTrainer.member_seed(7, 3) == member_seed(7, 3)


class _Fake:
    """Stands in for HipEnsembleTrainer: records what it is given, returns recognisable numbers."""
    made = []

    def __init__(self, weights_per_member, biases_per_member, act_codes, device=None, learning_rate=1e-3, rule="adam"):
        self.w = [[np.array(w) for w in ws] for ws in weights_per_member]          # copies: the handler writes the members later
        self.b = [[np.array(b) for b in bs] for bs in biases_per_member]
        self.acts = list(act_codes)
        self.device, self.lr, self.rule, self.closed = device, learning_rate, rule, False
        _Fake.made.append(self)

    def fit(self, train_in, train_out, val_in, val_out, epochs, batch_size, member_rows=None, permutations=None, generator_seed=None):
        self.fit_args = dict(train_in=train_in, train_out=train_out, val_in=val_in, val_out=val_out, epochs=epochs,
                             batch_size=batch_size, member_rows=member_rows, permutations=permutations, seed=generator_seed)
        E = len(self.w)
        return (np.arange(E * epochs, dtype=np.float64).reshape(E, epochs) + 100.0,
                np.arange(E * epochs, dtype=np.float64).reshape(E, epochs) + 200.0)

    def residual_rms(self, val_in, val_out):
        return np.asarray([[1.0, 2.0, 2.0], [2.0, 2.0, 4.0], [2.0, 2.0, 4.0]], F)

    def numpy_params(self, member):
        return ([np.full_like(w, member + 1) for w in self.w[member]], [np.full_like(b, -(member + 1)) for b in self.b[member]])

    def close(self):
        self.closed = True


def _handler(fn):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    return SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)


def test_the_handler_hands_rows_and_permutations_to_one_ensemble_trainer(built_lib, monkeypatch):
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    monkeypatch.setattr(T, "HipEnsembleTrainer", _Fake)
    monkeypatch.setattr(T, "HipDenseTrainer", None)             # the sequential path would fail loudly
    _Fake.made = []
    obs, acs, rews = _episodes(2, 20, 2, 0)
    fn = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=3, seed=0)
    start = [[w.copy() for w in m.weights] for m in fn.members]
    h = _handler(fn)
    seed, epochs = 5, 4
    h.train(obs, acs, rews, epochs=epochs, batch_size=8, learning_rate=3e-3, nn_optimizer="SGD", seed=seed, backend="hip")
    assert len(_Fake.made) == 1
    fake = _Fake.made[0]
    assert fake.closed and fake.rule == "sgd" and fake.lr == 3e-3 and fake.acts == list(fn.members[0].activation_codes)
    for e in range(3):
        for got, want in zip(fake.w[e], start[e]):
            np.testing.assert_array_equal(got, want)
    a = fake.fit_args
    n = h._model_training_in.shape[0]
    tin, tout = h._normalize_data(h._model_training_in, h._model_training_out)
    vin, vout = h._normalize_data(h._model_validation_in, h._model_validation_out)
    for got, want in ((a["train_in"], tin), (a["train_out"], tout), (a["val_in"], vin), (a["val_out"], vout)):
        np.testing.assert_array_equal(got, want)                # the rows once, not resampled
    assert a["epochs"] == epochs and a["batch_size"] == 8 and a["seed"] == seed
    assert len(a["member_rows"]) == 3 and len(a["permutations"]) == 3
    for e in range(3):                                          # the draws of the sequential loop, in its order
        rng = np.random.default_rng([seed, e])
        np.testing.assert_array_equal(a["member_rows"][e], rng.integers(0, n, size=n))
        np.testing.assert_array_equal(a["permutations"][e], [rng.permutation(n) for _ in range(epochs)])
    # what the fake returned, where the loop puts it
    for e, member in enumerate(fn.members):
        np.testing.assert_array_equal(h.member_training_loss[e], np.arange(epochs) + 100.0 + e * epochs)
        np.testing.assert_array_equal(h.member_validation_loss[e], np.arange(epochs) + 200.0 + e * epochs)
        assert all(np.all(w == e + 1) for w in member.weights) and all(np.all(b == -(e + 1)) for b in member.biases)
    np.testing.assert_array_equal(h.training_loss, h.member_training_loss[0])
    np.testing.assert_array_equal(h.validation_loss, h.member_validation_loss[0])
    np.testing.assert_array_equal(h._residual_rms, np.sqrt(np.asarray([9.0, 12.0, 36.0]) / 3.0).astype(F))
    assert h.residual_std().shape == (3,)
    # injected rows and permutations (one list shared by the members) go through as given
    _Fake.made = []
    fn = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=3, seed=1)
    h = _handler(fn)
    mask = np.arange(80) % 4 != 0
    n = int(mask.sum())
    rng = np.random.default_rng(3)
    boots = [rng.integers(0, n, size=n) for _ in range(3)]
    perms = [rng.permutation(n) for _ in range(2)]
    h.train(obs, acs, rews, epochs=2, batch_size=8, split_mask=mask, bootstrap_indices=boots, permutations=perms, backend="hip")
    a = _Fake.made[0].fit_args
    for e in range(3):
        np.testing.assert_array_equal(a["member_rows"][e], boots[e])
        np.testing.assert_array_equal(a["permutations"][e], perms)


def test_the_torch_backend_and_log_variance_ensembles_do_not_touch_it(built_lib, monkeypatch):
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    monkeypatch.setattr(T, "HipEnsembleTrainer", _Fake)
    _Fake.made = []
    obs, acs, rews = _episodes(1, 20, 2, 0)
    fn = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=0)
    h = _handler(fn)
    h.train(obs, acs, rews, epochs=1, batch_size=8, device="cpu", seed=0, backend="torch")
    assert not _Fake.made and len(h.member_training_loss) == 2 and np.isfinite(h.training_loss[0])
    fn = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=0, probabilistic=True)
    with pytest.raises(ValueError, match="backend='torch'"):
        _handler(fn).train(obs, acs, rews, epochs=1, batch_size=8, backend="hip")
    assert not _Fake.made
