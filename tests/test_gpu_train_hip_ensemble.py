"""All members of an ensemble in one launch sequence (bbmpc_trainer_create_ensemble / _fit_ensemble; csrc/kernels_train.hpp,
blockIdx.y = member; DESIGN.md section 8p, "Members") against the code it replaces: one HipDenseTrainer per member, fitted on
`train_in[rows[e]]`.  A member's arithmetic and summation order are by construction the single trainer's, so every value
comparison here is `assert_array_equal` -- there is no tolerance to choose.  Shapes are the smallest at which the kernels
take every path: one, two (the second with ONE live row, B = 17) and three tiles; 4-32-32-3 (whole tiles) and 7-20-33-5
(ragged tiles, a kept swish pre-activation); n_train no multiple of B (the remainder is dropped); E = 1, 2, 3 and the limit 8."""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests import train_hip_util as U
from tests.test_gpu_activations import CODE
from tests.test_train_cpu import _episodes

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NETS = {"4-32-32-3": ((4, 32, 32, 3), ("tanh", "tanh", None)),
        "7-20-33-5": ((7, 20, 33, 5), ("swish", "tanh", None))}
EPOCHS = 3


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


class Case:
    """E members of one network with distinct start weights, bootstrap rows and permutations, on shared rows."""

    def __init__(self, net, E, B, n_val, seed, epochs=EPOCHS):
        self.dims, self.acts = NETS[net]
        self.codes = [CODE[a] for a in self.acts]
        self.E, self.B, self.epochs = E, B, epochs
        n = 3 * B + 5                                           # three steps per epoch, five rows dropped
        rng = np.random.default_rng(seed)
        x, y = U.dataset(n + n_val, self.dims[0], self.dims[-1], seed=seed + 1)
        self.tin, self.tout, self.vin, self.vout = x[:n], y[:n], x[n:], y[n:]
        self.starts = [U.params(self.dims, seed=seed + 10 + e) for e in range(E)]
        self.rows = [rng.integers(0, n, size=n) for _ in range(E)]
        self.perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(E)]


def _sequential(c, rule="adam", lr=2e-3, perms="case", seeds=None, fits=1):
    """The yardstick: per member a HipDenseTrainer on tin[rows[e]].  Returns per member (weights + biases, train loss, val
    loss, residual RMS) after `fits` fits."""
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer
    out = []
    for e in range(c.E):
        tr = HipDenseTrainer(c.starts[e][0], c.starts[e][1], c.codes, None, learning_rate=lr, rule=rule)
        tr.set_data(c.tin[c.rows[e]], c.tout[c.rows[e]], c.vin, c.vout)
        for _ in range(fits):
            tl, vl = tr.fit_resident(c.epochs, c.B, permutations=c.perms[e] if perms == "case" else None,
                                     generator_seed=None if seeds is None else seeds[e])
        out.append((sum(tr.numpy_params(), []), tl, vl, tr.residual_rms(c.vin, c.vout)))
        tr.close()
    return out


def _ensemble_trainer(c, rule="adam", lr=2e-3):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipEnsembleTrainer
    return HipEnsembleTrainer([s[0] for s in c.starts], [s[1] for s in c.starts], c.codes, None, learning_rate=lr, rule=rule)


def _results(tr, tl, vl, c):
    rms = tr.residual_rms(c.vin, c.vout)
    return [(sum(tr.numpy_params(e), []), tl[e], vl[e], None if rms is None else rms[e]) for e in range(c.E)]


def _ensemble(c, rule="adam", lr=2e-3, perms="case", seed=None, fits=1):
    tr = _ensemble_trainer(c, rule, lr)
    tr.set_data(c.tin, c.tout, c.vin, c.vout, member_rows=c.rows)
    for _ in range(fits):
        tl, vl = tr.fit_resident(c.epochs, c.B, permutations=c.perms if perms == "case" else None, generator_seed=seed)
    out = _results(tr, tl, vl, c)
    tr.close()
    return out


def _assert_member_equal(got, want):
    for g, w in zip(got[0], want[0]):
        np.testing.assert_array_equal(g, w)                    # NaN == NaN here
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[2], want[2])
    if want[3] is None:
        assert got[3] is None
    else:
        np.testing.assert_array_equal(got[3], want[3])


def _assert_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        _assert_member_equal(g, w)


# ---- 1. members against sequential fits -------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,lr", [("adam", 2e-3), ("sgd", 1e-2), ("rmsprop", 1e-3)])
@pytest.mark.parametrize("B", [16, 17, 40])
@pytest.mark.parametrize("net", sorted(NETS))
@pytest.mark.parametrize("E", [1, 2, 3, 8])
def test_members_equal_sequential_fits(L, E, net, B, rule, lr):
    for n_val in (B + 3, B - 1):                                # one full validation batch; none: the loss is NaN
        c = Case(net, E, B, n_val, seed=1000 + 10 * E + B)
        want = _sequential(c, rule, lr)
        got = _ensemble(c, rule, lr)
        _assert_equal(got, want)
        for e in range(E):
            assert np.all(np.isfinite(got[e][1])) and got[e][3].shape == (c.dims[-1],)
            assert np.all(np.isnan(got[e][2])) if n_val < B else np.all(np.isfinite(got[e][2]))
        if E > 1:                                               # the members really are different fits
            assert not np.array_equal(got[0][0][0], got[1][0][0]) and not np.array_equal(got[0][1], got[1][1])


def test_two_validation_batches_and_the_fit_entry_point(L):
    c = Case("7-20-33-5", 3, 17, 2 * 17 + 4, seed=1500)
    want, got = _sequential(c), _ensemble(c)
    _assert_equal(got, want)
    # `fit` (set_data + set_member_rows + fit_ensemble), permutations as nested lists, is `fit_resident`
    tr = _ensemble_trainer(c)
    tl, vl = tr.fit(c.tin, c.tout, c.vin, c.vout, c.epochs, c.B, member_rows=c.rows, permutations=c.perms)
    assert tl.shape == vl.shape == (3, c.epochs)
    _assert_equal(_results(tr, tl, vl, c), want)
    assert tr.residual_rms(c.vin[:0], c.vout[:0]) is None
    tr.close()


# ---- 2. E = 1 and the library's own permutations ------------------------------------------------------------------------
def test_one_member_is_the_single_trainer(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer
    c = Case("7-20-33-5", 1, 17, 20, seed=2000)
    ws, bs = c.starts[0]
    for perms, seed in ((c.perms[0], None), (None, 77)):
        single = HipDenseTrainer(ws, bs, c.codes, None, learning_rate=2e-3)
        s_tl, s_vl = single.fit(c.tin, c.tout, c.vin, c.vout, c.epochs, c.B, permutations=perms, generator_seed=seed)
        ens = _ensemble_trainer(c)
        e_tl, e_vl = ens.fit(c.tin, c.tout, c.vin, c.vout, c.epochs, c.B, permutations=None if perms is None else [perms],
                             generator_seed=seed)                 # no member_rows: the identity
        _assert_member_equal((sum(ens.numpy_params(0), []), e_tl[0], e_vl[0], ens.residual_rms(c.vin, c.vout)[0]),
                             (sum(single.numpy_params(), []), s_tl, s_vl, single.residual_rms(c.vin, c.vout)))
        single.close()
        ens.close()


def test_library_permutations_follow_the_member_seed_rule(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import member_seed
    c = Case("4-32-32-3", 3, 16, 19, seed=2100)
    seed = 0xFEDCBA9876543210                                     # member 1 and 2 wrap past 2^64
    seeds = [member_seed(seed, e) for e in range(3)]
    assert seeds[0] == seed and len(set(seeds)) == 3
    _assert_equal(_ensemble(c, perms=None, seed=seed), _sequential(c, perms=None, seeds=seeds))


# ---- 3. isolation -----------------------------------------------------------------------------------------------------
def test_a_member_does_not_see_its_neighbours(L):
    c = Case("7-20-33-5", 3, 17, 20, seed=3000)
    base = _ensemble(c)
    other = Case("7-20-33-5", 3, 17, 20, seed=3001)
    c.starts[1], c.rows[1], c.perms[1] = other.starts[1], other.rows[1], other.perms[1]
    changed = _ensemble(c)
    _assert_member_equal(changed[0], base[0])
    _assert_member_equal(changed[2], base[2])
    assert not np.array_equal(changed[1][0][0], base[1][0][0])
    # NaN start weights in member 1: its results are NaN, its neighbours' bits stay
    c.starts[1] = ([w.copy() for w in c.starts[1][0]], c.starts[1][1])
    c.starts[1][0][0][0, 0] = np.nan
    poisoned = _ensemble(c)
    _assert_member_equal(poisoned[0], base[0])
    _assert_member_equal(poisoned[2], base[2])
    assert np.all(np.isnan(poisoned[1][1])) and np.all(np.isfinite(poisoned[0][1])) and np.all(np.isfinite(poisoned[2][1]))


def test_reversing_the_members_reverses_the_results(L):
    c = Case("4-32-32-3", 3, 40, 43, seed=3100)
    base = _ensemble(c, rule="rmsprop", lr=1e-3)
    c.starts, c.rows, c.perms = c.starts[::-1], c.rows[::-1], c.perms[::-1]
    _assert_equal(_ensemble(c, rule="rmsprop", lr=1e-3), base[::-1])


# ---- 4. repeatability and reuse -----------------------------------------------------------------------------------------
def test_equal_ensemble_fits_give_equal_bits(L):
    c = Case("7-20-33-5", 3, 40, 43, seed=4000)
    _assert_equal(_ensemble(c), _ensemble(c))


@pytest.mark.parametrize("rule,lr", [("adam", 2e-3), ("rmsprop", 1e-3)])
def test_a_second_fit_continues_every_members_optimizer_state(L, rule, lr):
    c = Case("4-32-32-3", 3, 17, 20, seed=4100)
    _assert_equal(_ensemble(c, rule, lr, fits=2), _sequential(c, rule, lr, fits=2))


# ---- 5. the handler -----------------------------------------------------------------------------------------------------
def _counting(monkeypatch):
    """Count the trainer handles of either kind made from here on."""
    from blackbox_mpc_amd.dynamics_functions import _train_hip as T
    made = {"single": 0, "ensemble": 0}
    for cls, key in ((T.HipDenseTrainer, "single"), (T.HipEnsembleTrainer, "ensemble")):
        def init(self, *a, _orig=cls.__init__, _key=key, **kw):
            made[_key] += 1
            _orig(self, *a, **kw)
        monkeypatch.setattr(cls, "__init__", init)
    return made


def _ensemble_handler(seed):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    fn = EnsembleMLP([4, 32, 32, 3], ["tanh", "tanh", None], num_members=3, seed=seed)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)
    return h, fn, [([w.copy() for w in m.weights], [b.copy() for b in m.biases]) for m in fn.members]


def _assert_handler_equals_sequential_fits(h, fn, start, boots, perms, epochs, B, lr):
    """The handler's results against explicit HipDenseTrainer fits on the rows the handler normalised."""
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer
    tin, tout = h._normalize_data(h._model_training_in, h._model_training_out)
    vin, vout = h._normalize_data(h._model_validation_in, h._model_validation_out)
    rms = []
    for e, member in enumerate(fn.members):
        tr = HipDenseTrainer(start[e][0], start[e][1], member.activation_codes, None, learning_rate=lr)
        tl, vl = tr.fit(tin[boots[e]], tout[boots[e]], vin, vout, epochs, B, permutations=perms[e])
        for got, want in zip(member.weights + member.biases, sum(tr.numpy_params(), [])):
            np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(h.member_training_loss[e], tl)
        np.testing.assert_array_equal(h.member_validation_loss[e], vl)
        rms.append(tr.residual_rms(vin, vout))
        tr.close()
    np.testing.assert_array_equal(h.training_loss, h.member_training_loss[0])
    np.testing.assert_array_equal(h.validation_loss, h.member_validation_loss[0])
    want = np.sqrt(np.mean(np.square(np.asarray(rms, np.float64)), axis=0)).astype(F) * (np.asarray(h._stats[5], F) + F(1e-7))
    np.testing.assert_array_equal(h.residual_std(), want.astype(F))


def test_the_handler_fits_an_ensemble_with_one_trainer(L, monkeypatch):
    obs, acs, rews = _episodes(3, 40, 2, 5)
    epochs, B, lr = 3, 32, 2e-3
    # injected draws
    h, fn, start = _ensemble_handler(6)
    rng = np.random.default_rng(7)
    mask = rng.random(3 * 40 * 2) > 0.25
    n = int(mask.sum())
    boots = [rng.integers(0, n, size=n) for _ in range(3)]
    perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(3)]
    made = _counting(monkeypatch)
    h.train(obs, acs, rews, batch_size=B, learning_rate=lr, epochs=epochs, split_mask=mask, permutations=perms,
            bootstrap_indices=boots, backend="hip")
    assert made == {"single": 0, "ensemble": 1}
    _assert_handler_equals_sequential_fits(h, fn, start, boots, perms, epochs, B, lr)
    assert not np.array_equal(fn.members[0].weights[0], fn.members[1].weights[0])
    # seed only: rows and permutations redrawn here from default_rng([seed, e])
    h, fn, start = _ensemble_handler(8)
    made.update(single=0, ensemble=0)
    h.train(obs, acs, rews, batch_size=B, learning_rate=lr, epochs=epochs, seed=11, backend="hip")
    assert made == {"single": 0, "ensemble": 1}
    n = h._model_training_in.shape[0]
    boots, perms = [], []
    for e in range(3):
        rng = np.random.default_rng([11, e])
        boots.append(rng.integers(0, n, size=n))
        perms.append([rng.permutation(n) for _ in range(epochs)])
    _assert_handler_equals_sequential_fits(h, fn, start, boots, perms, epochs, B, lr)


# ---- 6. refusals and lifecycle ------------------------------------------------------------------------------------------
def test_refusals_on_a_live_handle_leave_it_usable(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import _ptr_array
    c = Case("4-32-32-3", 2, 16, 19, seed=6000)
    want = _ensemble(c)
    n = c.tin.shape[0]
    tr = _ensemble_trainer(c)
    lib, t = L.lib, tr._t
    tl, vl = np.zeros((2, c.epochs), F), np.zeros((2, c.epochs), F)

    def refused(got, code, *words):
        msg = lib.bbmpc_last_error().decode()
        assert got == code and "trainer" in msg and all(w in msg for w in words), (got, msg)

    rows = np.ascontiguousarray(c.rows, np.int32)
    refused(lib.bbmpc_trainer_fit_ensemble(t, c.epochs, c.B, None, 0, L.ptr(tl), L.ptr(vl)), L.E_STATE, "bbmpc_trainer_set_data")
    refused(lib.bbmpc_trainer_set_member_rows(t, L.ptr(rows)), L.E_STATE, "bbmpc_trainer_set_data")
    tr.set_data(c.tin, c.tout, c.vin, c.vout, member_rows=c.rows)
    for B in (0, 4097):
        refused(lib.bbmpc_trainer_fit_ensemble(t, c.epochs, B, None, 0, L.ptr(tl), L.ptr(vl)), L.E_UNSUPPORTED, "batch_size")
    refused(lib.bbmpc_trainer_fit_ensemble(t, 0, c.B, None, 0, L.ptr(tl), L.ptr(vl)), L.E_INVALID, "epochs")
    refused(lib.bbmpc_trainer_fit_ensemble(t, c.epochs, c.B, None, 0, None, L.ptr(vl)), L.E_INVALID)
    refused(lib.bbmpc_trainer_fit_ensemble(t, c.epochs, c.B, None, 0, L.ptr(tl), None), L.E_INVALID)
    # the index array [E][epochs][n] has to stay below 2^31 entries: refused before it is built
    big = -(-(1 << 31) // (2 * n))
    assert 2 * big * n >= 1 << 31 > 2 * (big - 1) * n
    refused(lib.bbmpc_trainer_fit_ensemble(t, big, c.B, None, 0, L.ptr(tl), L.ptr(vl)), L.E_UNSUPPORTED, "too large")
    bad = np.ascontiguousarray(c.perms, np.int32)
    bad[1, 2, 5] = n                                            # member 1, last epoch: an entry outside the rows
    refused(lib.bbmpc_trainer_fit_ensemble(t, c.epochs, c.B, L.ptr(bad), 0, L.ptr(tl), L.ptr(vl)), L.E_INVALID, "permutation")
    bad_rows = rows.copy()
    bad_rows[1, 3] = -1
    refused(lib.bbmpc_trainer_set_member_rows(t, L.ptr(bad_rows)), L.E_INVALID, "row")      # ... and the map stays as it was
    ws = [np.zeros_like(w) for w in c.starts[0][0]]
    bs = [np.zeros_like(b) for b in c.starts[0][1]]
    for member in (-1, 2):
        refused(lib.bbmpc_trainer_get_member_params(t, member, _ptr_array(ws), _ptr_array(bs)), L.E_INVALID, "member")
    refused(lib.bbmpc_trainer_get_member_params(t, 0, None, _ptr_array(bs)), L.E_INVALID)
    rms = np.zeros((2, 3), F)
    refused(lib.bbmpc_trainer_residual_rms_ensemble(t, None, L.ptr(c.vout), 19, L.ptr(rms)), L.E_INVALID)
    refused(lib.bbmpc_trainer_residual_rms_ensemble(t, L.ptr(c.vin), L.ptr(c.vout), 0, L.ptr(rms)), L.E_INVALID, "row")
    # the single-member entry points on an ensemble: BBMPC_E_STATE, naming the call to use
    idx, g, loss = np.arange(16, dtype=np.int32), np.zeros(4 * 32 + 32 * 32 + 32 * 3 + 67, F), ctypes.c_float(0)
    refused(lib.bbmpc_trainer_fit(t, c.epochs, c.B, None, 0, L.ptr(tl), L.ptr(vl)), L.E_STATE, "bbmpc_trainer_fit_ensemble")
    refused(lib.bbmpc_trainer_get_params(t, _ptr_array(ws), _ptr_array(bs)), L.E_STATE, "bbmpc_trainer_get_member_params")
    refused(lib.bbmpc_trainer_residual_rms(t, L.ptr(c.vin), L.ptr(c.vout), 19, L.ptr(rms)), L.E_STATE, "bbmpc_trainer_residual_rms_ensemble")
    refused(lib.bbmpc_trainer_gradients(t, L.ptr(idx), 16, L.ptr(g), ctypes.byref(loss)), L.E_STATE, "ensemble")
    with pytest.raises(L.BBMPCError) as ei:                     # the Python restatement of the 2^31 bound
        tr.fit_resident(big, c.B, generator_seed=0)
    assert ei.value.code == L.E_UNSUPPORTED and "trainer" in str(ei.value)
    # nothing moved: the start weights are there bit for bit, and the fit is the fit of a handle that refused nothing
    for e in range(2):
        for got, start in zip(sum(tr.numpy_params(e), []), c.starts[e][0] + c.starts[e][1]):
            np.testing.assert_array_equal(got, start)
    tl, vl = tr.fit_resident(c.epochs, c.B, permutations=c.perms)
    _assert_equal(_results(tr, tl, vl, c), want)
    # a new set_data resets the member rows to the identity
    tr.close()
    c1 = Case("4-32-32-3", 2, 16, 19, seed=6000)
    c1.rows = [np.arange(n), np.arange(n)]
    tr = _ensemble_trainer(c1)
    tr.set_data(c.tin, c.tout, c.vin, c.vout, member_rows=c.rows)
    tr.set_data(c.tin, c.tout, c.vin, c.vout)
    tl, vl = tr.fit_resident(c.epochs, c.B, permutations=c.perms)
    _assert_equal(_results(tr, tl, vl, c1), _sequential(c1))
    tr.close()


def test_creation_refusals_of_the_ensemble_constructor(L):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipEnsembleTrainer
    ws, bs = U.params((4, 8, 3), seed=1)
    for E in (0, 9):
        with pytest.raises(L.BBMPCError) as ei:
            HipEnsembleTrainer([ws] * E, [bs] * E, [1, 0])
        assert ei.value.code == L.E_UNSUPPORTED and "trainer" in str(ei.value) and "n_members" in str(ei.value)
    with pytest.raises(ValueError, match="member 1"):
        HipEnsembleTrainer([ws, [ws[0], ws[1][:, :2]]], [bs, [bs[0], bs[1][:2]]], [1, 0])
    assert L.lib.bbmpc_trainer_fit_ensemble(None, 1, 16, None, 0, None, None) == L.E_INVALID


def test_create_and_destroy_fifty_ensemble_trainers(L):
    c = Case("4-32-32-3", 8, 16, 0, seed=6100)
    for _ in range(50):
        _ensemble_trainer(c).close()


# ---- 7. the example and the rate print --------------------------------------------------------------------------------
def test_the_example_runs_in_its_smallest_setting(L):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "train_hip_ensemble_pendulum.py"), "--small"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "one HIP ensemble fit" in res.stdout and "control steps through the ensemble" in res.stdout


def test_fit_time_of_five_members_through_both_paths(L, capsys):
    """Unasserted: one timed 5-member fit, one trainer per member against one launch sequence (tools/train_rate.py measures)."""
    from oracle import oracle_np as O
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipDenseTrainer, HipEnsembleTrainer
    rng = np.random.default_rng(0)
    n, E, B, epochs = 8192, 5, 128, 2
    din, dout = rng.normal(size=(n, 26)).astype(F), rng.normal(size=(n, 20)).astype(F)
    starts = [O.make_mlp_params([26, 200, 200, 20], seed=1 + e) for e in range(E)]
    rows = [rng.integers(0, n, size=n) for _ in range(E)]

    def sequential(seed):
        for e in range(E):
            tr = HipDenseTrainer(starts[e][0], starts[e][1], [1, 1, 0], None)
            tl, _ = tr.fit(din[rows[e]], dout[rows[e]], din[:256], dout[:256], epochs, B, generator_seed=seed)
            tr.close()
        return tl

    def one_launch(seed):
        tr = HipEnsembleTrainer([s[0] for s in starts], [s[1] for s in starts], [1, 1, 0], None)
        tl, _ = tr.fit(din, dout, din[:256], dout[:256], epochs, B, member_rows=rows, generator_seed=seed)
        tr.close()
        return tl

    took = {}
    for name, fn in (("sequential", sequential), ("one launch", one_launch)):
        fn(0)
        t0 = time.perf_counter()
        tl = fn(1)
        took[name] = time.perf_counter() - t0
        assert np.all(np.isfinite(tl))
    steps = E * epochs * (n // B)
    with capsys.disabled():
        print("\n[train_hip] 5-member fit, 26-200-200-20, batch 128, %d member-steps incl. upload: one HipDenseTrainer per member "
              "%.4f s (%.0f member-steps/s), HipEnsembleTrainer %.4f s (%.0f member-steps/s)"
              % (steps, took["sequential"], steps / took["sequential"], took["one launch"], steps / took["one launch"]))
