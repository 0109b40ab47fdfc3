"""What tests/test_gpu_train_hip_shapes.py takes for granted, proved without a GPU on the float64 reference alone: every
committed integer case is exact in float32 whatever the order of summation, the reference's kink conventions are the
kernels', every committed saturating case covers every branch and keeps clear of the kinks, the cases meant for the LDS
carve over 64 KiB and for the wave-strided loops' second trip really are such cases, and `train(..., opt=...)` is
oracle_train.train when the optimizer is fresh."""
import numpy as np
import pytest

from oracle import oracle_train as OT
from tests import train_hip_util as U
from tests.test_gpu_activations import CODE

F = np.float32
ALL_INTEGER = dict(U.INTEGER_CASES, **U.RAGGED_CASES)


@pytest.mark.parametrize("name", list(ALL_INTEGER))
def test_integer_cases_are_exact_in_float32(name):
    dims, acts, B, seed, nnz = ALL_INTEGER[name]
    ws, bs, x, y = U.integer_case(dims, acts, B, seed, nnz)
    assert x.shape == (B, dims[0]) and y.shape == (B, dims[-1])
    for a in ws + bs + [x, y]:
        assert a.dtype == F and np.array_equal(a, np.rint(a))
    assert set(np.unique(x)) <= {-2, -1, 0, 1, 2} and all(set(np.unique(w)) <= {-1, 0, 1} for w in ws)
    bounds = U.integer_exactness(ws, bs, acts, x, y)
    n = len(ws)
    assert set(bounds) == {"sq"} | {"z%d" % l for l in range(n)} | {"dW%d" % l for l in range(n)} | \
        {"db%d" % l for l in range(n)} | {"g%d" % l for l in range(1, n)}
    assert max(bounds.values()) < 2 ** 24                       # the bound of the issue, not one fitted to the cases
    # the float32 casts the GPU test compares with lose nothing: every gradient is an integer times 2 / (B O)
    loss, gw, gb = U.mse_and_grads(ws, bs, list(acts), x, y)
    half = B * dims[-1] / 2.0
    pow2 = (B * dims[-1]) & (B * dims[-1] - 1) == 0
    assert pow2 == (name in U.INTEGER_CASES)
    if pow2:
        for g in gw + gb:
            assert np.array_equal(g * half, np.rint(g * half)) and np.array_equal(g.astype(F).astype(np.float64), g)
        assert float(F(loss)) == loss
    # every layer says something: no all-zero gradient
    assert all(np.count_nonzero(g) for g in gw + gb)


def test_the_reference_takes_the_kernels_branch_at_the_kinks():
    """Integer pre-activations sit ON the kinks.  train_act_grad gives relu at 0 the derivative 0 (x > 0 asked with x = y)
    and relu6 at 0 and at 6 the derivative 0 (y > 0 && y < 6); the reference must say the same there."""
    z = np.array([-1.0, 0.0, 1.0, 5.0, 6.0, 7.0])
    f, d = U._act("relu")
    np.testing.assert_array_equal(d(z, f(z)), [0, 0, 1, 1, 1, 1])
    f, d = U._act("relu6")
    np.testing.assert_array_equal(d(z, f(z)), [0, 0, 1, 1, 0, 0])
    hit = {"relu": 0, "relu6": 0}                                 # ... and the cases do reach them, after layer 0 too
    for dims, acts, B, seed, nnz in ALL_INTEGER.values():
        ws, bs, x, y = U.integer_case(dims, acts, B, seed, nnz)
        zs = U.forward(ws, bs, acts, x)[1]
        for l, a in enumerate(acts):
            if a is not None and l > 0:
                hit[a] += int(np.sum(zs[l] == 0.0) + (np.sum(zs[l] == 6.0) if a == "relu6" else 0))
    assert hit["relu"] > 0 and hit["relu6"] > 0


def test_integer_cases_cover_the_shapes_they_are_there_for(built_lib):
    from blackbox_mpc_amd.dynamics_functions._train_hip import lds_bytes, lds_bytes_formula
    cases = U.INTEGER_CASES
    for name in U.LDS_OVER_64K:
        dims, acts = cases[name][0], [CODE[a] for a in cases[name][1]]
        assert lds_bytes_formula(dims, acts) > 64 * 1024 and lds_bytes(dims, acts) == lds_bytes_formula(dims, acts)
        assert lds_bytes(dims, acts) <= 159 * 1024
        assert max(dims) > 256                                  # more than 16 tiles: the wave-strided loops take a second trip
    widths = {d for c in cases.values() for d in c[0]}
    assert {1, 15, 16, 17, 255, 256, 257, 512} <= widths
    assert {c[2] for c in cases.values()} >= {1, 2, 16, 32, 64, 4096}
    assert {c[0][-1] for c in cases.values()} >= {32, 64, 128}
    depths = {len(c[1]) for c in cases.values()}
    assert 1 in depths and 8 in depths
    assert any(c[1][-1] is not None for c in cases.values())    # an activation on the last layer
    assert {c[2] for c in U.RAGGED_CASES.values()} == {5, 17, 33}


@pytest.mark.parametrize("act", sorted(CODE, key=lambda k: CODE[k]))
def test_saturating_cases_cover_every_branch_and_keep_clear_of_the_kinks(act):
    assert len(CODE) == 13
    ws, bs, acts, x, y = U.saturating_case(act, U.SAT_SEED_OF.get(act, U.SAT_SEED))          # asserts both conditions
    assert acts == (act, act, None) and x.shape == (U.SAT_ROWS, 6) and y.shape == (U.SAT_ROWS, 3)
    assert all(a.dtype == F for a in ws + bs + [x, y])
    ys, zs = U.forward(ws, bs, acts, x)
    z = np.concatenate([zs[0].ravel(), zs[1].ravel()])            # restated here, so the helper cannot quietly stop asserting
    half = 4.0 if act == "exponential" else 9.0
    assert np.all(np.isfinite(ys[-1])) and 0.8 * half <= np.max(np.abs(z)) <= 1.5 * half
    if act in U.KINKS:
        edges = (-np.inf,) + U.KINKS[act] + (np.inf,)
        shares = [float(np.mean((z > lo) & (z < hi))) for lo, hi in zip(edges[:-1], edges[1:])]
        assert min(shares) >= 0.10, shares
        assert min(float(np.min(np.abs(z - k))) for k in U.KINKS[act]) >= 1e-3
    else:
        far = 2.0 if act == "exponential" else 4.0
        assert np.mean(z > far) >= 0.10 and np.mean(z < -far) >= 0.10
    # the 1e-3 margin against float32: the same forward in float32 lands within 1e-5 of the reference
    y32 = x
    for l in range(2):
        z32 = y32 @ ws[l] + bs[l]
        assert np.max(np.abs(z32.astype(np.float64) - zs[l])) < 1e-5
        y32 = ys[l + 1].astype(F)


def test_kinks_name_every_piecewise_code():
    assert set(U.KINKS) == {"relu", "relu6", "leaky_relu", "hard_sigmoid", "elu", "selu"}
    assert U.KINKS["relu6"] == (0.0, 6.0) and U.KINKS["hard_sigmoid"] == (-2.5, 2.5)


@pytest.mark.parametrize("rule", ["adam", "sgd", "rmsprop"])
def test_train_with_a_carried_optimizer_is_the_oracles_train(rule):
    dims, acts = (4, 20, 3), ["tanh", None]
    ws, bs = U.params(dims, seed=1)
    x, y = U.dataset(80, 4, 3, seed=2)
    perms = [np.random.default_rng(3 + e).permutation(64) for e in range(3)]
    want = OT.train(ws, bs, acts, x[:64], y[:64], x[64:], y[64:], perms, batch_size=16, learning_rate=2e-3, rule=rule)
    # a fresh optimizer handed in: the same numbers
    got = U.train(ws, bs, acts, x[:64], y[:64], x[64:], y[64:], perms, 16, learning_rate=2e-3, rule=rule,
                  opt=U.optimizer(rule, ws, bs, 2e-3))
    for a, b in zip(got[0] + got[1] + [got[2], got[3]], want[0] + want[1] + [want[2], want[3]]):
        np.testing.assert_array_equal(a, b)
    # one epoch, then two with the same optimizer: the three-epoch fit
    opt = U.optimizer(rule, ws, bs, 2e-3)
    first = U.train(ws, bs, acts, x[:64], y[:64], x[64:], y[64:], perms[:1], 16, learning_rate=2e-3, rule=rule, opt=opt)
    second = U.train(first[0], first[1], acts, x[:64], y[:64], x[64:], y[64:], perms[1:], 16, learning_rate=2e-3, rule=rule, opt=opt)
    for a, b in zip(second[0] + second[1], want[0] + want[1]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.concatenate([first[2], second[2]]), want[2])
    np.testing.assert_array_equal(np.concatenate([first[3], second[3]]), want[3])
