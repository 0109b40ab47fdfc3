"""The HIP Dense trainer (csrc/kernels_train.hpp, bbmpc_trainer_*, HipDenseTrainer) where tests/test_gpu_train_hip.py
stops: wide, deep, ragged and saturated shapes.

1. exact arithmetic: small-integer networks whose every float32 product and partial sum is exact in any order (proved on the
   reference in tests/test_train_hip_shapes_cpu.py), so gradients and loss equal the float64 reference bit for bit --
   through every tile edge, L = 1 and L = 8, B = 1 .. 4096, multi-tile outputs, widths over 256 (the wave-strided loops'
   second trip) and the LDS carve over 64 KiB;
2. real-valued gradients with test_gradients_against_the_float64_oracle's measure and yardstick: the widest network, an
   activation on the last layer, B < 16 and ragged, and every activation code driven into its saturated / negative branches;
3. the three layouts k_train_update writes, against packs the host builds from the same parameters, by bits;
4. optimizer state across calls: split fits, a gradients() call between them, set_data again, a larger batch later;
5. residual_rms and validation over ragged rows and wide outputs."""
import time

import numpy as np
import pytest

from tests import train_hip_util as U
from tests.test_gpu_activations import CODE
from tests.test_gpu_train_hip import LOSS_ATOL, LOSS_RTOL, W_ATOL, _assert_fit_matches, _fit_case, _torch_gradients, _trainer

pytestmark = pytest.mark.gpu
F = np.float32
_START = []


@pytest.fixture(scope="module")
def L():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib
    assert _lib.device_count() >= 1
    _START.append(time.perf_counter())
    return _lib


def _flat(tr):
    ws, bs = tr.numpy_params()
    return ws + bs


def _assert_same_bits(a, b):
    assert len(a) == len(b)
    for p, q in zip(a, b):
        np.testing.assert_array_equal(np.asarray(p), np.asarray(q))


# ---- 1. exact arithmetic ----------------------------------------------------------------------------------------------
def _integer_gradients(case, exact_scaling=False):
    """((loss, dW, db) of the trainer, the same of U.mse_and_grads) on the case's whole batch.  exact_scaling: where B O is
    no power of two the reference's own 2 diff / (B O) rounds too (at 1e-16, but a sum that cancels to an exact zero then
    reads 1e-17); its gradients are integers times 2 / (B O), so they are rounded back to those integers and scaled once."""
    dims, acts, B, seed, nnz = case
    ws, bs, x, y = U.integer_case(dims, acts, B, seed, nnz)
    tr = _trainer(ws, bs, acts)
    tr.set_data(x, y, x[:0], y[:0])
    got = tr.gradients(np.arange(B))
    want = U.mse_and_grads(ws, bs, list(acts), x, y)
    tr.close()
    if exact_scaling:
        half = B * dims[-1] / 2.0
        assert all(np.max(np.abs(g * half - np.rint(g * half))) < 1e-9 for g in want[1] + want[2])
        want = (want[0], [np.rint(g * half) / half for g in want[1]], [np.rint(g * half) / half for g in want[2]])
    return got, want


@pytest.mark.parametrize("name", list(U.INTEGER_CASES))
def test_integer_networks_give_the_reference_gradient_exactly(L, name):
    """Zero tolerance: on this data float32 arithmetic is exact in any order, so a wrong lane, a transposed index, a
    dropped or doubled tile or a read of padding is a different integer."""
    from blackbox_mpc_amd.dynamics_functions._train_hip import lds_bytes_formula
    dims, acts = U.INTEGER_CASES[name][:2]
    if name in U.LDS_OVER_64K:                                              # the case keeps covering that branch
        assert lds_bytes_formula(dims, [CODE[a] for a in acts]) > 64 * 1024
    (loss, gw, gb), (want_loss, ww, wb) = _integer_gradients(U.INTEGER_CASES[name])
    for l, (got, want) in enumerate(zip(gw + gb, ww + wb)):
        np.testing.assert_array_equal(got, want.astype(F), err_msg="tensor %d of %s" % (l, name))
    assert F(loss) == F(want_loss)


# B O is no power of two here, so 2 / (B O) is no float32 and the product with it rounds.  That is the ONLY rounding: the
# kernels sum the exact integer terms first and k_train_update scales each sum once (DESIGN.md 8p says what scaling every
# delta first cost: 5.85 ulp at B = 17).  Two roundings of half an ulp each, whatever cancels in the sum: a few ulp.
RAGGED_RTOL = 2.0 ** -22


@pytest.mark.parametrize("name", list(U.RAGGED_CASES))
def test_integer_networks_at_ragged_batch_sizes(L, name, capsys):
    (loss, gw, gb), (want_loss, ww, wb) = _integer_gradients(U.RAGGED_CASES[name], exact_scaling=True)
    worst = []
    for got, want in zip(gw + gb, ww + wb):
        nz = want != 0
        worst.append(float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0)
    with capsys.disabled():
        print("\n[train_hip] integer case %s: worst |got - want| / |want| per tensor (in units of 2^-24): %s; loss %.2f"
              % (name, ", ".join("%.2f" % (w * 2 ** 24) for w in worst), abs(loss - want_loss) / want_loss * 2 ** 24))
    for got, want in zip(gw + gb, ww + wb):
        np.testing.assert_allclose(got, want, rtol=RAGGED_RTOL, atol=0)
    np.testing.assert_allclose(loss, want_loss, rtol=RAGGED_RTOL, atol=0)


# ---- 2. real-valued gradients -----------------------------------------------------------------------------------------
def _check_gradients(capsys, label, ws, bs, acts, x, y, idx):
    """test_gradients_against_the_float64_oracle's measure and yardstick on the batch x[idx], y[idx]."""
    tr = _trainer(ws, bs, acts)
    tr.set_data(x, y, x[:0], y[:0])
    loss, gw, gb = tr.gradients(idx)
    tr.close()
    want_loss, ww, wb = U.mse_and_grads(ws, bs, list(acts), x[idx], y[idx])
    t_loss, tw, tb = _torch_gradients(ws, bs, [CODE[a] for a in acts], x[idx], y[idx])
    rows = []
    for name, got, tor, want in [("W%d" % l, gw[l], tw[l], ww[l]) for l in range(len(ws))] + \
                                [("b%d" % l, gb[l], tb[l], wb[l]) for l in range(len(ws))]:
        rows.append((name, U.rel_err(got, want), U.rel_err(tor, want)))
    with capsys.disabled():
        print("\n[train_hip] gradient error %s B=%d (max|got-want|/max|want|; hip / torch): %s; loss %.3e / %.3e"
              % (label, len(idx), ", ".join("%s %.2e / %.2e" % r for r in rows), abs(loss - want_loss) / want_loss,
                 abs(t_loss - want_loss) / want_loss))
    assert all(np.all(np.isfinite(g)) for g in gw + gb)
    for name, e_hip, e_torch in rows:
        assert e_hip <= max(4.0 * e_torch, 1e-6), (name, e_hip, e_torch)
    assert abs(loss - want_loss) <= max(4.0 * abs(t_loss - want_loss), 1e-6 * want_loss)


def _random_case(capsys, dims, acts, B, seed):
    ws, bs = U.params(dims, seed=seed)
    x, y = U.dataset(max(B, 64), dims[0], dims[-1], seed=seed + 1, offset=0.5)     # (why the offset: train_hip_util.dataset)
    idx = np.random.default_rng(seed + 2).permutation(x.shape[0])[:B]
    _check_gradients(capsys, "-".join(map(str, dims)) + " " + "/".join(str(a) for a in acts), ws, bs, acts, x, y, idx)


@pytest.mark.parametrize("B", [16, 40])
def test_gradients_of_the_widest_network(L, B, capsys):
    _random_case(capsys, (26, 500, 500, 500, 20), ("tanh", "tanh", "tanh", None), B, seed=200)


@pytest.mark.parametrize("dims", [(46, 300, 1), (9, 257, 100)])
def test_gradients_with_swish_then_sigmoid_on_the_last_layer(L, dims, capsys):
    _random_case(capsys, dims, ("swish", "sigmoid"), 24, seed=210)


@pytest.mark.parametrize("last", ["tanh", "sigmoid", "softplus", "swish", "exponential"])
def test_gradients_with_a_nonlinear_last_layer(L, last, capsys):
    _random_case(capsys, (7, 20, 33, 5), ("swish", "tanh", last), 24, seed=220)


@pytest.mark.parametrize("B", [1, 5, 17])
def test_gradients_of_batches_below_and_across_a_tile(L, B, capsys):
    _random_case(capsys, (7, 20, 33, 1), ("swish", "tanh", None), B, seed=230)


@pytest.mark.parametrize("act", sorted(CODE, key=lambda k: CODE[k]))
def test_gradients_in_the_saturated_branches_of_every_activation(L, act, capsys):
    ws, bs, acts, x, y = U.saturating_case(act, U.SAT_SEED_OF.get(act, U.SAT_SEED))
    _check_gradients(capsys, "saturated " + str(act), ws, bs, acts, x, y, np.arange(U.SAT_ROWS))


# ---- 3. the layouts k_train_update writes -----------------------------------------------------------------------------
@pytest.mark.parametrize("rule,lr", [("adam", 2e-3), ("sgd", 1e-2), ("rmsprop", 1e-3)])
@pytest.mark.parametrize("dims,acts", [((17, 33, 15, 2), ("swish", "tanh", None)), ((4, 300, 3), ("tanh", None))])
def test_updated_packs_are_the_packs_of_the_updated_parameters(L, dims, acts, rule, lr):
    """After three steps the first trainer reads wf, wr and the padded bias as k_train_update wrote them; a trainer built from
    its parameters reads packs the host laid out.  The same batch must give the same bits."""
    ws, bs = U.params(dims, seed=300)
    x, y = U.dataset(48, dims[0], dims[-1], seed=301)
    tr = _trainer(ws, bs, acts, learning_rate=lr, rule=rule)
    tr.fit(x, y, x[:0], y[:0], 1, 16, permutations=[np.random.default_rng(302).permutation(48)])      # three steps
    idx = np.random.default_rng(303).permutation(48)[:24]
    loss, gw, gb = tr.gradients(idx)
    w1, b1 = tr.numpy_params()
    assert not np.array_equal(w1[0], ws[0])
    other = _trainer(w1, b1, acts, learning_rate=lr, rule=rule)
    other.set_data(x, y, x[:0], y[:0])
    loss2, gw2, gb2 = other.gradients(idx)
    _assert_same_bits(gw + gb + [F(loss)], gw2 + gb2 + [F(loss2)])
    _assert_same_bits(_flat(other), w1 + b1)
    assert np.isfinite(loss) and all(np.count_nonzero(g) for g in gw + gb)


# ---- 4. state across calls --------------------------------------------------------------------------------------------
def _split_case(n_rows):
    dims, acts = (4, 20, 3), ("tanh", None)
    ws, bs = U.params(dims, seed=400)
    x, y = U.dataset(n_rows + 32, 4, 3, seed=401)
    perms = [np.random.default_rng(402 + e).permutation(n_rows) for e in range(3)]
    return dims, acts, ws, bs, x[:n_rows], y[:n_rows], x[n_rows:], y[n_rows:], perms


@pytest.mark.parametrize("between", [False, True], ids=["", "gradients-between"])
@pytest.mark.parametrize("n_rows", [64, 48])                     # 4 steps per epoch; 3: the first call ends on an odd step
@pytest.mark.parametrize("rule", ["adam", "rmsprop"])
def test_a_fit_in_two_calls_is_the_fit_in_one(L, rule, n_rows, between):
    dims, acts, ws, bs, tin, tout, vin, vout, perms = _split_case(n_rows)
    whole = _trainer(ws, bs, acts, learning_rate=2e-3, rule=rule)
    tl, vl = whole.fit(tin, tout, vin, vout, 3, 16, permutations=perms)
    split = _trainer(ws, bs, acts, learning_rate=2e-3, rule=rule)
    tl1, vl1 = split.fit(tin, tout, vin, vout, 1, 16, permutations=perms[:1])
    if between:
        before = _flat(split)
        split.gradients(np.arange(16))
        _assert_same_bits(_flat(split), before)
    tl2, vl2 = split.fit(tin, tout, vin, vout, 2, 16, permutations=perms[1:])
    _assert_same_bits(_flat(split) + [np.concatenate([tl1, tl2]), np.concatenate([vl1, vl2])], _flat(whole) + [tl, vl])
    want = U.train(ws, bs, list(acts), tin, tout, vin, vout, perms, batch_size=16, learning_rate=2e-3, rule=rule)
    _assert_fit_matches(whole, (tl, vl), want)


def test_set_data_again_with_other_rows(L):
    dims, acts = (4, 20, 3), ("tanh", None)
    ws, bs = U.params(dims, seed=410)
    xa, ya = U.dataset(64 + 32, 4, 3, seed=411)
    xb, yb = U.dataset(100 + 50, 4, 3, seed=412)
    pa = [np.random.default_rng(413 + e).permutation(64) for e in range(2)]
    pb = [np.random.default_rng(415 + e).permutation(100) for e in range(2)]
    tr = _trainer(ws, bs, acts, learning_rate=1e-2, rule="sgd")                 # sgd keeps no state: a fresh trainer can follow
    tr.fit(xa[:64], ya[:64], xa[64:], ya[64:], 2, 16, permutations=pa)
    wa, ba = tr.numpy_params()
    got = tr.fit(xb[:100], yb[:100], xb[100:], yb[100:], 2, 24, permutations=pb)
    fresh = _trainer(wa, ba, acts, learning_rate=1e-2, rule="sgd")
    want = fresh.fit(xb[:100], yb[:100], xb[100:], yb[100:], 2, 24, permutations=pb)
    _assert_same_bits(_flat(tr) + list(got), _flat(fresh) + list(want))
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and not np.array_equal(_flat(tr)[0], wa[0])
    oracle = U.train(wa, ba, list(acts), xb[:100], yb[:100], xb[100:], yb[100:], pb, batch_size=24, learning_rate=1e-2, rule="sgd")
    _assert_fit_matches(tr, got, oracle)


@pytest.mark.parametrize("rule", ["adam", "rmsprop"])
def test_a_larger_batch_on_a_later_call(L, rule):
    """B = 16, then B = 128 on the same trainer: the share buffers grow between the calls, m, v and the step count carry."""
    dims, acts = (4, 20, 3), ("tanh", None)
    ws, bs = U.params(dims, seed=420)
    x, y = U.dataset(256 + 128, 4, 3, seed=421)
    tin, tout, vin, vout = x[:256], y[:256], x[256:], y[256:]
    p1 = [np.random.default_rng(422).permutation(256)]
    p2 = [np.random.default_rng(423 + e).permutation(256) for e in range(2)]
    tr = _trainer(ws, bs, acts, learning_rate=2e-3, rule=rule)
    l1 = tr.fit(tin, tout, vin, vout, 1, 16, permutations=p1)
    l2 = tr.fit(tin, tout, vin, vout, 2, 128, permutations=p2)
    opt = U.optimizer(rule, ws, bs, 2e-3)
    o1 = U.train(ws, bs, list(acts), tin, tout, vin, vout, p1, 16, learning_rate=2e-3, rule=rule, opt=opt)
    o2 = U.train(o1[0], o1[1], list(acts), tin, tout, vin, vout, p2, 128, learning_rate=2e-3, rule=rule, opt=opt)
    np.testing.assert_allclose(l1[0], o1[2], rtol=LOSS_RTOL, atol=LOSS_ATOL)
    np.testing.assert_allclose(l1[1], o1[3], rtol=LOSS_RTOL, atol=LOSS_ATOL)
    _assert_fit_matches(tr, l2, o2)
    # a fresh optimizer for the second call would not pass: the state does carry
    o2_fresh = U.train(o1[0], o1[1], list(acts), tin, tout, vin, vout, p2, 128, learning_rate=2e-3, rule=rule)
    assert max(float(np.max(np.abs(a - b))) for a, b in zip(o2_fresh[0], o2[0])) > 4 * W_ATOL


# ---- 5. residual_rms and validation -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 17, 250])
@pytest.mark.parametrize("O", [1, 33, 100])
def test_residual_rms_over_ragged_rows_and_wide_outputs(L, O, n):
    dims, acts = (5, 20, O), ("tanh", None)
    ws, bs = U.params(dims, seed=500 + O)
    x, y = U.dataset(n, 5, O, seed=501 + O)
    tr = _trainer(ws, bs, acts)
    d = y.astype(np.float64) - U.forward(ws, bs, acts, x)[0][-1]
    got = tr.residual_rms(x, y)
    assert got.shape == (O,)
    np.testing.assert_allclose(got, np.sqrt(np.mean(d * d, axis=0)), rtol=1e-4, atol=1e-6)


def test_fit_with_a_wide_output_and_left_over_validation_rows(L):
    tr, losses, want = _fit_case((5, 20, 100), ("tanh", None), 100, 80, 24, 3, "adam", 2e-3, seed=510)    # 80 = 3 x 24 + 8
    assert np.all(np.isfinite(want[3]))
    _assert_fit_matches(tr, losses, want)
    x, y = U.dataset(180, 5, 100, seed=511)                                  # _fit_case's rows; the last 80 validate
    x, y = x[100:], y[100:]
    w, b = tr.numpy_params()
    d = y.astype(np.float64) - U.forward(w, b, ("tanh", None), x)[0][-1]
    np.testing.assert_allclose(tr.residual_rms(x, y), np.sqrt(np.mean(d * d, axis=0)), rtol=1e-4, atol=1e-6)


def test_wall_time_of_this_file(L, capsys):
    with capsys.disabled():
        print("\n[train_hip] tests/test_gpu_train_hip_shapes.py: %.1f s from its first test to its last" % (time.perf_counter() - _START[0]))
