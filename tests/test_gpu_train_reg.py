"""Weight decay, early stopping and best-weights restore in the hand-written training kernels (csrc/kernels_train.hpp,
bbmpc_trainer_set_weight_decay / _set_early_stopping / _get_fit_report) on the GPU.

Shapes are the smallest that reach the index paths: 4-8-3 (below one tile) and 17-33-5 (every width crosses a tile edge, so
the hoisted layer lookup and the pack writers see ragged layers), batches of 16 and 17 rows (one tile and two), ensembles
of 1, 2 and 3 members, at most 6 epochs.  Bit comparisons wherever the rule allows them; the two comparisons against the
float64 statement (tests/train_reg_util.py) use tests/test_gpu_train_hip.py's tolerances for a fit against the oracle."""
import ctypes

import numpy as np
import pytest

from tests import train_hip_util as U
from tests import train_reg_util as RU
from tests.test_gpu_activations import CODE
from tests.test_gpu_train_hip import LOSS_ATOL, LOSS_RTOL, W_ATOL
from tests.test_train_cpu import _episodes

pytestmark = pytest.mark.gpu
F = np.float32
NETS = {"4-8-3": ((4, 8, 3), ("tanh", None), 16), "17-33-5": ((17, 33, 5), ("tanh", None), 17)}
RULES = [("adam", 2e-2), ("sgd", 5e-2), ("rmsprop", 1e-2)]


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


def _ensemble(wss, bss, acts, **kw):
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipEnsembleTrainer
    return HipEnsembleTrainer(wss, bss, [CODE[a] for a in acts], None, **kw)


def _flat(tr, member=None):
    ws, bs = tr.numpy_params() if member is None else tr.numpy_params(member)
    return ws + bs


def _same_bits(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(np.asarray(p), np.asarray(q))


def _case(net, seed=5, batches=2, val_batches=1, epochs=6):
    """(acts, B, weights, biases, train rows, validation rows, permutations): `batches` full batches and a dropped
    remainder of 2 rows per epoch."""
    dims, acts, B = NETS[net]
    ws, bs = U.params(dims, seed)
    n = batches * B + 2
    x, y = U.dataset(n + val_batches * B, dims[0], dims[-1], seed + 1)
    rng = np.random.default_rng(seed + 2)
    perms = [rng.permutation(n) for _ in range(epochs)]
    return acts, B, ws, bs, (x[:n], y[:n]), (x[n:], y[n:]), perms


def _fit(tr, train, val, epochs, B, perms):
    return tr.fit(train[0], train[1], val[0], val[1], epochs, B, permutations=perms[:epochs])


# ---- 1. defaults ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,lr", RULES)
@pytest.mark.parametrize("net", sorted(NETS))
def test_options_set_to_their_defaults_change_no_bit(L, net, rule, lr):
    acts, B, ws, bs, train, val, perms = _case(net)
    plain = _trainer(ws, bs, acts, learning_rate=lr, rule=rule)
    want = _fit(plain, train, val, 3, B, perms)
    told = _trainer(ws, bs, acts, learning_rate=lr, rule=rule)
    told.set_weight_decay([0.0, 0.0], "decoupled")                  # the library is called, with nothing to do
    told.set_early_stopping(0, 0.0, False)
    got = _fit(told, train, val, 3, B, perms)
    _same_bits(_flat(told), _flat(plain))
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert (told.epochs_run, told.best_epoch) == (3, -1) and np.isnan(told.best_val)
    assert (plain.epochs_run, plain.best_epoch) == (3, -1)


# ---- 2. exact arithmetic ----------------------------------------------------------------------------------------------
def _exact_case():
    """tests/train_hip_util.integer_case at 17-33-5, B = 17, made exact although B O = 85 is no power of two: the targets are
    moved so that every output error is a multiple of 85.  Every summed gradient S is then a multiple of 85 too and the
    kernel's one rounding, S * float32(2 / 85), has the integer 2 S / 85 to land on -- asserted below in float32 on the
    float64 reference's gradients, for this data.  With lr and lambda powers of two every further product and sum is exact
    (a few bits below 2^-9, a few above 1), in float32 as in float64."""
    dims, acts, B = (17, 33, 5), ("relu6", None), 17
    ws, bs, x, _ = U.integer_case(dims, acts, B, 131, 4)
    rng = np.random.default_rng(132)
    out = U.forward(ws, bs, acts, x)[0][-1]
    y = (out - 85.0 * rng.integers(-1, 2, size=out.shape)).astype(F)
    U.integer_exactness(ws, bs, acts, x, y)
    _, gw, gb = U.mse_and_grads(ws, bs, list(acts), x, y)
    for g in gw + gb:
        s = np.rint(g * 85.0 / 2.0)
        np.testing.assert_array_equal(s * 2.0 / 85.0, g)            # integers times 2 / 85 ...
        np.testing.assert_array_equal((s.astype(F) * F(2.0 / 85.0)).astype(np.float64), g)      # ... which float32 scaling reaches
    assert all(np.count_nonzero(g) for g in gw)
    return acts, B, ws, bs, x, y


@pytest.mark.parametrize("mode", ["l2", "decoupled"])
def test_one_decayed_sgd_step_is_the_float64_statement_exactly(L, mode):
    acts, B, ws, bs, x, y = _exact_case()
    lr, decay = 2.0 ** -6, [2.0 ** -3, 0.0]
    perm = [np.arange(B)]
    tr = _trainer(ws, bs, acts, learning_rate=lr, rule="sgd", weight_decay=decay, decay_mode=mode)
    tr.fit(x, y, x[:0], y[:0], 1, B, permutations=perm)
    w, b = RU.train(ws, bs, acts, x, y, x[:0], y[:0], perm, B, lr, "sgd", weight_decay=decay, decay_mode=mode)[:2]
    for got, want in zip(_flat(tr), w + b):
        np.testing.assert_array_equal(got, want.astype(F))
        np.testing.assert_array_equal(got.astype(np.float64), want)             # the statement's values ARE float32 values here
    plain = _trainer(ws, bs, acts, learning_rate=lr, rule="sgd")
    plain.fit(x, y, x[:0], y[:0], 1, B, permutations=perm)
    np.testing.assert_array_equal(tr.numpy_params()[0][1], plain.numpy_params()[0][1])      # lambda_1 = 0: the undecayed bits
    assert np.count_nonzero(tr.numpy_params()[0][0] != plain.numpy_params()[0][0]) > 100   # lambda_0 moved the nonzero weights
    _same_bits(tr.numpy_params()[1], plain.numpy_params()[1])


@pytest.mark.parametrize("net", sorted(NETS))
def test_a_zero_data_gradient_shrinks_the_kernels_and_nothing_else(L, net):
    acts, B, ws, bs, train, val, perms = _case(net, batches=3)
    ws[-1][:], bs[-1][:] = 0.0, 0.0                                 # f(x) = 0 = the targets: the data gradient is exactly 0
    zeros = np.zeros_like(train[1])
    lr, lam = 2.0 ** -3, 2.0 ** -2
    tr = _trainer(ws, bs, acts, learning_rate=lr, rule="sgd", weight_decay=lam, decay_mode="l2")
    tl, _ = tr.fit(train[0], zeros, val[0][:0], val[1][:0], 1, B, permutations=perms[:1])       # 3 steps
    assert tl[0] == 0.0
    gw, gb = tr.numpy_params()
    want = RU.shrink_f32(ws[0], lr, lam, 3)
    np.testing.assert_array_equal(gw[0], want)
    assert np.all(want != ws[0])
    np.testing.assert_array_equal(gw[1], ws[1])                     # zeros stay zeros
    _same_bits(gb, bs)


# ---- 3. adam and rmsprop with decay against the float64 statement ------------------------------------------------------
@pytest.mark.parametrize("rule,lr", [("adam", 2e-2), ("rmsprop", 1e-2)])
@pytest.mark.parametrize("mode", ["l2", "decoupled"])
@pytest.mark.parametrize("net", sorted(NETS))
def test_decayed_fits_match_the_float64_statement(L, net, mode, rule, lr):
    acts, B, ws, bs, train, val, perms = _case(net, batches=3)
    decay = [0.5, 0.25]
    tr = _trainer(ws, bs, acts, learning_rate=lr, rule=rule, weight_decay=decay, decay_mode=mode)
    tl, vl = _fit(tr, train, val, 2, B, perms)
    w, b, wtl, wvl, _ = RU.train(ws, bs, acts, train[0], train[1], val[0], val[1], perms[:2], B, lr, rule, weight_decay=decay,
                                 decay_mode=mode)
    for got, want in zip(_flat(tr), w + b):
        np.testing.assert_allclose(got, want, rtol=0, atol=W_ATOL)
    np.testing.assert_allclose(tl, wtl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(vl, wvl, rtol=LOSS_RTOL, atol=LOSS_ATOL)
    plain = RU.train(ws, bs, acts, train[0], train[1], val[0], val[1], perms[:2], B, lr, rule)[0]
    other = RU.train(ws, bs, acts, train[0], train[1], val[0], val[1], perms[:2], B, lr, rule, weight_decay=decay,
                     decay_mode="l2" if mode == "decoupled" else "decoupled")[0]
    assert max(np.max(np.abs(p - x)) for p, x in zip(plain, w)) > 10 * W_ATOL        # the case tells decay from none ...
    assert max(np.max(np.abs(o - x)) for o, x in zip(other, w)) > 3 * W_ATOL         # ... and the modes from each other


# ---- 4. members equal singles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 2, 3])
@pytest.mark.parametrize("net", sorted(NETS))
def test_members_equal_single_trainers(L, net, E):
    acts, B, _, _, train, val, _ = _case(net, seed=254, val_batches=2)
    dims, n, epochs = NETS[net][0], train[0].shape[0], 6
    rng = np.random.default_rng(77)
    starts = [U.params(dims, 300 + e) for e in range(E)]
    rows = [rng.integers(0, n, size=n) for _ in range(E)]
    perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(E)]
    kw = dict(learning_rate=0.2, rule="adam", weight_decay=[1e-2, 0.0], decay_mode="decoupled", patience=1, min_delta=1e-3, restore_best=True)
    ens = _ensemble([s[0] for s in starts], [s[1] for s in starts], acts, **kw)
    tl, vl = ens.fit(train[0], train[1], val[0], val[1], epochs, B, member_rows=rows, permutations=perms)
    for e in range(E):
        one = _trainer(starts[e][0], starts[e][1], acts, **kw)
        otl, ovl = one.fit(train[0][rows[e]], train[1][rows[e]], val[0], val[1], epochs, B, permutations=perms[e])
        _same_bits(_flat(ens, e), _flat(one))
        np.testing.assert_array_equal(tl[e], otl)                   # NaN tails included
        np.testing.assert_array_equal(vl[e], ovl)
        assert (int(ens.epochs_run[e]), int(ens.best_epoch[e])) == (one.epochs_run, one.best_epoch)
        np.testing.assert_array_equal(ens.best_val[e], one.best_val)
        ran = one.epochs_run
        assert np.all(np.isfinite(otl[:ran])) and np.all(np.isnan(otl[ran:])) and np.all(np.isnan(ovl[ran:]))
        assert 0 <= one.best_epoch < ran and one.best_val == ovl[one.best_epoch]


# ---- 5. stopping and restoring ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,lr", RULES)
@pytest.mark.parametrize("net", sorted(NETS))
def test_a_forced_stop(L, net, rule, lr):
    acts, B, ws, bs, train, val, perms = _case(net)
    kw = dict(learning_rate=lr, rule=rule)
    free = {}
    for epochs in (1, 3):
        tr = _trainer(ws, bs, acts, **kw)
        free[epochs] = (_fit(tr, train, val, epochs, B, perms), _flat(tr))
    for restore, like in ((False, 3), (True, 1)):
        tr = _trainer(ws, bs, acts, patience=2, min_delta=1e9, restore_best=restore, **kw)
        tl, vl = _fit(tr, train, val, 6, B, perms)
        assert (tr.epochs_run, tr.best_epoch) == (3, 0) and tr.best_val == vl[0]
        np.testing.assert_array_equal(tl[:3], free[3][0][0])
        np.testing.assert_array_equal(vl[:3], free[3][0][1])
        assert np.all(np.isnan(tl[3:])) and np.all(np.isnan(vl[3:]))
        _same_bits(_flat(tr), free[like][1])
        if restore:                                                 # every layout the step kernel reads came back too
            fresh = _trainer(*tr.numpy_params(), acts)
            np.testing.assert_array_equal(tr.residual_rms(*val), fresh.residual_rms(*val))
            fresh.set_data(train[0], train[1], val[0], val[1])
            got, want = tr.gradients(np.arange(B)), fresh.gradients(np.arange(B))
            assert got[0] == want[0]
            _same_bits(got[1] + got[2], want[1] + want[2])


def test_a_stopped_member_does_not_disturb_the_others(L):
    acts, B, _, _, train, val, perms = _case("17-33-5")
    dims = NETS["17-33-5"][0]
    starts = [U.params(dims, 400 + e) for e in range(3)]
    broken = ([np.full_like(w, np.nan) for w in starts[1][0]], [np.full_like(b, np.nan) for b in starts[1][1]])
    kw = dict(learning_rate=2e-2, rule="adam", weight_decay=1e-2, patience=2, restore_best=True)
    out = {}
    for name, middle in (("finite", starts[1]), ("nan", broken)):
        members = [starts[0], middle, starts[2]]
        ens = _ensemble([m[0] for m in members], [m[1] for m in members], acts, **kw)
        losses = ens.fit(train[0], train[1], val[0], val[1], 6, B, permutations=perms)
        out[name] = (ens, losses)
    ens, (tl, vl) = out["nan"]
    assert (int(ens.epochs_run[1]), int(ens.best_epoch[1])) == (2, -1) and np.isnan(ens.best_val[1])
    assert np.all(np.isnan(tl[1])) and np.all(np.isnan(vl[1]))
    assert all(np.all(np.isnan(p)) for p in _flat(ens, 1))          # nothing to restore: the weights stay what the steps left
    ref, (rtl, rvl) = out["finite"]
    for e in (0, 2):
        _same_bits(_flat(ens, e), _flat(ref, e))
        np.testing.assert_array_equal(tl[e], rtl[e])
        np.testing.assert_array_equal(vl[e], rvl[e])
        assert (ens.epochs_run[e], ens.best_epoch[e], ens.best_val[e]) == (ref.epochs_run[e], ref.best_epoch[e], ref.best_val[e])
        assert np.all(np.isfinite(tl[e][:int(ens.epochs_run[e])]))


def test_a_natural_interior_minimum_is_found_and_restored(L):
    """The data (17-33-5, 36 noisy rows, adam at 0.2, seed 254) were chosen on the host with DenseTrainer(device="cpu"): its
    free run's validation losses are 1.777 0.928 0.654 0.814 0.864 0.806 -- the minimum at epoch 2, every other epoch at
    least 23 % above it, so float32 differences between the backends cannot move the argmin."""
    acts, B, ws, bs, train, val, perms = _case("17-33-5", seed=254, val_batches=2)
    kw = dict(learning_rate=0.2, rule="adam")
    free = _trainer(ws, bs, acts, **kw)
    _, vl = _fit(free, train, val, 6, B, perms)
    k = int(np.argmin(vl))
    assert 1 <= k <= 4, vl
    assert np.all(np.delete(vl, k) >= 1.01 * vl[k]), vl
    assert np.all(np.diff(vl[:k + 1]) < 0), vl                      # patience 1 walks down to it
    tr = _trainer(ws, bs, acts, patience=1, restore_best=True, **kw)
    tl, svl = _fit(tr, train, val, 6, B, perms)
    assert (tr.best_epoch, tr.epochs_run) == (k, k + 2) and tr.best_val == vl[k]
    np.testing.assert_array_equal(svl[:k + 2], vl[:k + 2])
    assert np.all(np.isnan(svl[k + 2:])) and np.all(np.isnan(tl[k + 2:]))
    best = _trainer(ws, bs, acts, **kw)
    _fit(best, train, val, k + 1, B, perms)
    _same_bits(_flat(tr), _flat(best))


# ---- 6. settings persist ----------------------------------------------------------------------------------------------
def test_settings_persist_until_they_are_switched_off(L):
    acts, B, ws, bs, train, val, perms = _case("17-33-5")
    kw = dict(learning_rate=5e-2, rule="sgd")                       # sgd keeps no state: a fresh trainer can follow a fit
    tr = _trainer(ws, bs, acts, weight_decay=[0.5, 0.25], patience=2, min_delta=1e9, restore_best=True, **kw)
    tr.set_data(train[0], train[1], val[0], val[1])
    tr.fit_resident(6, B, permutations=perms)
    assert (tr.epochs_run, tr.best_epoch) == (3, 0)
    first = _flat(tr)
    assert all(np.all(np.isfinite(p)) for p in first)
    tr.fit_resident(6, B, permutations=perms)                       # the same settings, from where the first fit ended
    assert (tr.epochs_run, tr.best_epoch) == (3, 0)
    again = _trainer(first[:2], first[2:], acts, weight_decay=[0.5, 0.25], patience=2, min_delta=1e9, restore_best=True, **kw)
    _fit(again, train, val, 6, B, perms)
    _same_bits(_flat(tr), _flat(again))
    plain = _trainer(first[:2], first[2:], acts, **kw)
    _fit(plain, train, val, 1, B, perms)
    assert any(np.any(p != q) for p, q in zip(_flat(tr), _flat(plain)))             # the decay was on in the second fit
    # off again: the bits of a trainer that never heard of them
    second = _flat(tr)
    tr.set_weight_decay(0.0)
    tr.set_early_stopping()
    tl, vl = tr.fit_resident(6, B, permutations=perms)
    assert (tr.epochs_run, tr.best_epoch) == (6, -1) and np.all(np.isfinite(tl)) and np.all(np.isfinite(vl))
    plain = _trainer(second[:2], second[2:], acts, **kw)
    ptl, pvl = _fit(plain, train, val, 6, B, perms)
    _same_bits(_flat(tr), _flat(plain))
    np.testing.assert_array_equal(tl, ptl)
    np.testing.assert_array_equal(vl, pvl)


def test_adam_goes_on_from_its_own_step_count_after_a_stop(L):
    """A stopped member's later launches leave m, v and the step count alone: fitted again, it continues like a trainer
    that ran exactly its epochs."""
    acts, B, ws, bs, train, val, perms = _case("4-8-3")
    kw = dict(learning_rate=2e-2, rule="adam")
    tr = _trainer(ws, bs, acts, patience=1, min_delta=1e9, **kw)     # stops after epoch 1: 4 steps of the 12 enqueued
    tr.set_data(train[0], train[1], val[0], val[1])
    tr.fit_resident(6, B, permutations=perms)
    assert tr.epochs_run == 2
    tr.set_early_stopping()
    tr.fit_resident(1, B, permutations=perms[2:3])
    free = _trainer(ws, bs, acts, **kw)
    _fit(free, train, val, 3, B, perms)
    _same_bits(_flat(tr), _flat(free))


# ---- 7. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(L):
    acts, B, ws, bs, train, val, perms = _case("4-8-3")
    tr = _trainer(ws, bs, acts, learning_rate=2e-2, rule="sgd", weight_decay=[0.5, 0.25], patience=3, min_delta=0.0)
    i32, f32 = lambda: np.zeros((1,), np.int32), lambda: np.zeros((1,), F)
    rep = (i32(), i32(), f32())

    def refused(code, expect, *words):
        assert code == expect, (code, expect)
        msg = L.lib.bbmpc_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(L.lib.bbmpc_trainer_get_fit_report(tr._t, *[L.ptr(a) for a in rep]), L.E_STATE, "bbmpc_trainer_get_fit_report", "before any fit")
    for decay in ([-1e-3, 0.0], [0.0, np.nan], [np.inf, 0.0]):
        refused(L.lib.bbmpc_trainer_set_weight_decay(tr._t, L.ptr(np.asarray(decay, F)), L.TRAIN_DECAY_L2), L.E_INVALID, "weight decay",
                "finite and >= 0")
    refused(L.lib.bbmpc_trainer_set_weight_decay(tr._t, L.ptr(np.zeros((2,), F)), 2), L.E_INVALID, "unknown weight decay mode")
    refused(L.lib.bbmpc_trainer_set_weight_decay(tr._t, None, -1), L.E_INVALID, "unknown weight decay mode")
    refused(L.lib.bbmpc_trainer_set_early_stopping(tr._t, -1, 0.0, 0), L.E_INVALID, "patience")
    for bad in (-1.0, float("nan"), float("inf")):
        refused(L.lib.bbmpc_trainer_set_early_stopping(tr._t, 1, bad, 1), L.E_INVALID, "min_delta")
    refused(L.lib.bbmpc_trainer_get_fit_report(tr._t, None, L.ptr(rep[1]), L.ptr(rep[2])), L.E_INVALID, "null")
    # monitoring without a full validation batch, single and ensemble entry point; nothing ran
    tl, vl = np.zeros((2,), F), np.zeros((2,), F)
    L.check(L.lib.bbmpc_trainer_set_data(tr._t, L.ptr(train[0]), L.ptr(train[1]), train[0].shape[0], L.ptr(val[0]), L.ptr(val[1]), B - 1))
    for fit in (L.lib.bbmpc_trainer_fit, L.lib.bbmpc_trainer_fit_ensemble):
        refused(fit(tr._t, 2, B, None, ctypes.c_uint64(0), L.ptr(tl), L.ptr(vl)), L.E_STATE, "validation", "no full batch")
    refused(L.lib.bbmpc_trainer_get_fit_report(tr._t, *[L.ptr(a) for a in rep]), L.E_STATE, "before any fit")
    _same_bits(_flat(tr), ws + bs)
    # every refusal left the settings as the constructor made them, and the trainer works
    got = _fit(tr, train, val, 2, B, perms)
    ref = _trainer(ws, bs, acts, learning_rate=2e-2, rule="sgd", weight_decay=[0.5, 0.25], patience=3, min_delta=0.0)
    want = _fit(ref, train, val, 2, B, perms)
    _same_bits(_flat(tr), _flat(ref))
    np.testing.assert_array_equal(got[1], want[1])
    w = RU.train(ws, bs, acts, train[0], train[1], val[0], val[1], perms[:2], B, 2e-2, "sgd", weight_decay=[0.5, 0.25], patience=3)
    for p, q in zip(_flat(tr), w[0] + w[1]):
        np.testing.assert_allclose(p, q, rtol=0, atol=W_ATOL)
    assert (tr.epochs_run, tr.best_epoch) == (w[4]["epochs_run"], w[4]["best_epoch"])
    with pytest.raises(ValueError, match="validation"):             # the Python surface refuses the same fit itself
        tr.fit(train[0], train[1], val[0][:B - 1], val[1][:B - 1], 2, B, permutations=perms)


# ---- 8. the handler ---------------------------------------------------------------------------------------------------
def test_the_handler_installs_the_restored_members(L):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions._train_hip import HipEnsembleTrainer
    from blackbox_mpc_amd.dynamics_functions.ensemble_mlp import EnsembleMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    obs, acs, rews = _episodes(2, 30, 2, 3)
    fn = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=1)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn)
    mask = np.random.default_rng(9).random(120) > 0.3
    h.train(obs, acs, rews, batch_size=16, learning_rate=0.1, epochs=6, seed=4, split_mask=mask, backend="hip",
            weight_decay=[1e-3, 0.0], patience=1, min_delta=1e9, restore_best=True)
    assert h.member_best_epoch == [0, 0] and h.member_epochs_run == [2, 2] and (h.epochs_run, h.best_epoch) == (2, 0)
    for e in range(2):
        assert np.all(np.isfinite(h.member_validation_loss[e][:2])) and np.all(np.isnan(h.member_validation_loss[e][2:]))
    # residual_std() is that of the installed (restored) weights: a fresh trainer holding them gives the same RMS
    vin, vout = h._normalize_data(h._model_validation_in, h._model_validation_out)
    tr = HipEnsembleTrainer([m.weights for m in fn.members], [m.biases for m in fn.members], fn.members[0].activation_codes)
    rms = tr.residual_rms(vin, vout)
    want = np.sqrt(np.mean(np.square(rms.astype(np.float64)), axis=0)).astype(F) * (np.asarray(h._stats[5], F) + F(1e-7))
    np.testing.assert_array_equal(h.residual_std(), want.astype(F))
    # and they are epoch 0's weights, not epoch 1's: a free one-epoch fit from the same start and draws gives the same bits
    fn1 = EnsembleMLP([4, 8, 3], ["tanh", None], num_members=2, seed=1)
    h1 = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn1)
    h1.train(obs, acs, rews, batch_size=16, learning_rate=0.1, epochs=1, seed=4, split_mask=mask, backend="hip", weight_decay=[1e-3, 0.0])
    assert h1.member_best_epoch == [-1, -1] and h1.member_epochs_run == [1, 1]
    for m, m1 in zip(fn.members, fn1.members):
        _same_bits(list(m.weights) + list(m.biases), list(m1.weights) + list(m1.biases))
