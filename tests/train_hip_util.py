"""Float64 restatements for the tests of the HIP training kernels (csrc/kernels_train.hpp) -- TEST INFRASTRUCTURE ONLY.

* `tile_decomposition`: the batch gradient as the kernels form it -- per 16-row tile a share of dW, db and of the sum of
  squared errors, rows past B contributing zeros, the shares added in ascending tile order.
* `mse_and_grads` / `train`: oracle_train's, for every activation code: oracle_train.ACTS where it has the code, the float64
  NumPy forms below otherwise.
* `params`, `dataset`, `rel_err`: what the GPU tests share.
"""
import numpy as np

from oracle import oracle_train as OT

F = np.float32
SELU_A, SELU_L = 1.6732632423543772, 1.0507009873554805
TILE = 16


def _sigma(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


# name -> (f(x), f'(x) from the pre-activation x and the output y): the TF 2.0 definitions, kinks as DenseTrainer._act_grad
ACTS64 = {
    "elu": (lambda x: np.where(x > 0, x, np.expm1(x)), lambda x, y: np.where(x > 0, 1.0, y + 1.0)),
    "selu": (lambda x: SELU_L * np.where(x > 0, x, SELU_A * np.expm1(x)),
             lambda x, y: np.where(x > 0, SELU_L, y + SELU_L * SELU_A)),
    "softplus": (lambda x: np.logaddexp(0.0, x), lambda x, y: _sigma(x)),
    "softsign": (lambda x: x / (1.0 + np.abs(x)), lambda x, y: 1.0 / np.square(1.0 + np.abs(x))),
    "exponential": (np.exp, lambda x, y: y),
    "hard_sigmoid": (lambda x: np.clip(0.2 * x + 0.5, 0.0, 1.0), lambda x, y: 0.2 * ((y > 0) & (y < 1))),
    "swish": (lambda x: x * _sigma(x), lambda x, y: _sigma(x) + y * (1.0 - _sigma(x))),
    "leaky_relu": (lambda x: np.where(x >= 0, x, 0.2 * x), lambda x, y: np.where(x > 0, 1.0, 0.2)),
    "relu6": (lambda x: np.clip(x, 0.0, 6.0), lambda x, y: 1.0 * ((y > 0) & (y < 6))),
}


def _act(name):
    """(f(x), f'(x, y)) in float64."""
    if name in OT.ACTS:
        f, d = OT.ACTS[name]
        return f, (lambda x, y: d(y))
    return ACTS64[name]


def forward(weights, biases, acts, x):
    """Layer outputs [x, y_1 .. y_L] and pre-activations [z_1 .. z_L], float64."""
    ys, zs = [np.asarray(x, np.float64)], []
    for w, b, a in zip(weights, biases, acts):
        zs.append(ys[-1] @ np.asarray(w, np.float64) + np.asarray(b, np.float64))
        ys.append(_act(a)[0](zs[-1]))
    return ys, zs


def _backprop(weights, acts, ys, zs, g):
    n = len(weights)
    gw, gb = [None] * n, [None] * n
    for l in reversed(range(n)):
        g = g * _act(acts[l])[1](zs[l], ys[l + 1])
        gw[l] = ys[l].T @ g
        gb[l] = g.sum(axis=0)
        g = g @ np.asarray(weights[l], np.float64).T
    return gw, gb


def mse_and_grads(weights, biases, acts, x, y):
    """oracle_train.mse_and_grads where it knows every activation; the same arithmetic with ACTS64 otherwise."""
    if all(a in OT.ACTS for a in acts):
        return OT.mse_and_grads([np.asarray(w, np.float64) for w in weights], [np.asarray(b, np.float64) for b in biases],
                                list(acts), np.asarray(x, np.float64), np.asarray(y, np.float64))
    ys, zs = forward(weights, biases, acts, x)
    diff = ys[-1] - np.asarray(y, np.float64)
    gw, gb = _backprop(weights, acts, ys, zs, 2.0 * diff / diff.size)
    return float(np.mean(diff * diff)), gw, gb


def tile_decomposition(weights, biases, acts, x, y):
    """(loss, dW, db) of the batch (x, y) as ceil(B / 16) tiles of 16 rows: rows past B are zero rows whose delta is zero,
    every tile gives a share of dW, db and of the squared-error sum, the shares are added in ascending tile order."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    B, O = y.shape
    tiles = (B + TILE - 1) // TILE
    gw = [np.zeros(np.shape(w), np.float64) for w in weights]
    gb = [np.zeros(np.shape(b), np.float64) for b in biases]
    sq = 0.0
    for t in range(tiles):
        live = np.zeros((TILE, 1))
        rows = slice(t * TILE, min((t + 1) * TILE, B))
        n = rows.stop - rows.start
        live[:n] = 1.0
        xt, yt = np.zeros((TILE, x.shape[1])), np.zeros((TILE, O))
        xt[:n], yt[:n] = x[rows], y[rows]
        ys, zs = forward(weights, biases, acts, xt)
        diff = (ys[-1] - yt) * live
        sq = sq + float(np.sum(diff * diff))
        sw, sb = _backprop(weights, acts, ys, zs, 2.0 * diff / (B * O))
        gw = [a + s for a, s in zip(gw, sw)]
        gb = [a + s for a, s in zip(gb, sb)]
    return sq / (B * O), gw, gb


def optimizer(rule, weights, biases, learning_rate):
    """A fresh oracle_train optimizer over (weights + biases): the state `train(..., opt=...)` carries from call to call."""
    return OT.OPTIMIZERS[rule]([np.array(x, np.float64) for x in list(weights) + list(biases)], learning_rate)


def train(weights, biases, acts, train_in, train_out, val_in, val_out, permutations, batch_size, learning_rate=1e-3, rule="adam",
          opt=None):
    """oracle_train.train where it knows every activation; otherwise its loop over `mse_and_grads` above.  With `opt` (from
    `optimizer`) the same loop steps that optimizer instead of a fresh one: m, v and the step count of a trainer that is
    fitted more than once."""
    if opt is None and all(a in OT.ACTS for a in acts):
        return OT.train(weights, biases, list(acts), train_in, train_out, val_in, val_out, permutations, batch_size=batch_size,
                        learning_rate=learning_rate, rule=rule)
    w = [np.array(x, np.float64) for x in weights]
    b = [np.array(x, np.float64) for x in biases]
    if opt is None:
        opt = OT.OPTIMIZERS[rule](w + b, learning_rate)
    tl, vl = [], []
    for perm in permutations:
        nb, acc = 0, 0.0
        for s in range(0, len(perm) - batch_size + 1, batch_size):
            idx = perm[s:s + batch_size]
            loss, gw, gb = mse_and_grads(w, b, acts, train_in[idx], train_out[idx])
            opt.step(w + b, gw + gb)
            acc += loss
            nb += 1
        tl.append(acc / nb if nb else np.nan)
        nb, acc = 0, 0.0
        for s in range(0, val_in.shape[0] - batch_size + 1, batch_size):
            d = forward(w, b, acts, val_in[s:s + batch_size])[0][-1] - val_out[s:s + batch_size]
            acc += float(np.mean(d * d))
            nb += 1
        vl.append(acc / nb if nb else np.nan)
    return w, b, np.array(tl), np.array(vl)


def rel_err(got, want):
    """max |got - want| / max |want| of one tensor."""
    want = np.asarray(want, np.float64)
    return float(np.max(np.abs(np.asarray(got, np.float64) - want)) / np.max(np.abs(want)))


def params(dims, seed):
    """Glorot kernels and small random biases, float32."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = np.sqrt(6.0 / (i + o))
        ws.append(rng.uniform(-lim, lim, size=(i, o)).astype(F))
        bs.append(rng.normal(0.0, 0.05, size=(o,)).astype(F))
    return ws, bs


def dataset(n, d_in, d_out, seed, offset=0.0):
    """Normalised-looking rows: x ~ N(0, 1), y a smooth function of x plus noise (plus `offset`).
    With centred targets the last layer's bias gradient, 2 mean(f(x) - y), is a cancelled sum of terms of either sign; on a
    one-output network that is a ONE-element tensor, and max |got - want| / max |want| of it then reports the conditioning
    of the data (sum |terms| / |sum terms|), whoever computes it.  The gradient test therefore shifts the targets by 0.5:
    the terms keep one sign on average and every tensor's measure is about the arithmetic."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, d_in)).astype(F)
    a = rng.normal(size=(d_in, d_out)) / np.sqrt(d_in)
    y = (np.tanh(x.astype(np.float64) @ a) + 0.1 * rng.normal(size=(n, d_out)) + offset).astype(F)
    return x, y


# ---- exact-arithmetic cases -------------------------------------------------------------------------------------------
EXACT = float(2 ** 24)                           # every integer below it is a float32
# name -> (dims, acts, B, seed, nonzeros per weight column).  B * O is a power of two in every case, so 2 / (B O) and
# 1 / (B O) scale exactly.  relu6 keeps the wide layers' outputs in [0, 6]: that, the column sparsity and the depth are
# what hold the bounds of `integer_exactness`; a case that missed them would get other integers, not a wider bound.
INTEGER_CASES = {
    "1-1-1 B16": ((1, 1, 1), ("relu", None), 16, 101, 1),
    "15-17-16 B16": ((15, 17, 16), ("relu6", None), 16, 102, 4),
    "16-16-16 B32": ((16, 16, 16), ("relu", "relu6"), 32, 103, 4),
    "17-15-1 B1": ((17, 15, 1), ("relu6", None), 1, 105, 4),
    "17-15-1 B2": ((17, 15, 1), ("relu", None), 2, 104, 4),
    "33-31-32 B64": ((33, 31, 32), ("relu", None), 64, 106, 4),
    "255-257-4 B16": ((255, 257, 4), ("relu6", None), 16, 107, 8),
    "512-256-2 B32": ((512, 256, 2), ("relu", None), 32, 108, 8),
    "4-512-512-8 B16": ((4, 512, 512, 8), ("relu6", "relu6", None), 16, 109, 8),
    "32-512-512-512-16 B32": ((32, 512, 512, 512, 16), ("relu6", "relu", "relu6", None), 32, 110, 8),
    "40-8 B16 (L=1)": ((40, 8), (None,), 16, 111, 6),
    "40-8 B2 (L=1, relu6)": ((40, 8), ("relu6",), 2, 112, 6),
    "9-17x7-4 B16 (L=8)": ((9,) + (17,) * 7 + (4,), ("relu", None, "relu6", "relu", None, "relu6", "relu", None), 16, 113, 3),
    "4-20-4 B4096": ((4, 20, 4), ("relu", None), 4096, 114, 3),
    "6-33-64 B16": ((6, 33, 64), ("relu6", None), 16, 115, 4),
    "6-33-128 B32": ((6, 33, 128), ("relu", "relu6"), 32, 116, 4),
    "5-20-65-128 B64": ((5, 20, 65, 128), ("relu", "relu6", None), 64, 117, 4),
}
LDS_OVER_64K = ("4-512-512-8 B16", "32-512-512-512-16 B32")      # the carve the step kernel needs its attribute raised for
# batch sizes whose B * O is no power of two: the same integers, a few ulp (test_gpu_train_hip_shapes says why)
RAGGED_CASES = {
    "7-20-33-1 B5": ((7, 20, 33, 1), ("relu", "relu6", None), 5, 121, 4),
    "7-20-33-1 B17": ((7, 20, 33, 1), ("relu", "relu6", None), 17, 122, 4),
    "17-33-3 B33": ((17, 33, 3), ("relu6", None), 33, 123, 4),
}


def integer_exactness(weights, biases, acts, x, y):
    """The largest integer any order of summation can meet in the forward and backward pass of this case, per product, from
    the float64 reference alone: (|A| @ |B|).max() of every matrix product, the backward quantities times B O / 2 (they are
    integers times 2 / (B O)), and the squared-error sum.  Asserts that every operand is an integer and every bound is below
    2^24: every float32 product and partial sum is then exact whatever the order, and (B O a power of two) so are the two
    scalings.  Returns {name: bound}."""
    assert all(a in (None, "relu", "relu6") for a in acts), acts
    w = [np.asarray(m, np.float64) for m in weights]
    b = [np.asarray(v, np.float64) for v in biases]
    ys, zs = forward(w, b, acts, x)
    y = np.asarray(y, np.float64)
    for a in w + b + ys + zs + [y]:
        assert np.array_equal(a, np.rint(a))
    out = {}
    n = len(w)
    for l in range(n):
        out["z%d" % l] = float((np.abs(ys[l]) @ np.abs(w[l]) + np.abs(b[l])).max())
    diff = ys[-1] - y
    out["sq"] = float(np.sum(diff * diff))
    g = diff                                                    # B O / 2 times the reference's 2 diff / (B O)
    for l in reversed(range(n)):
        g = g * _act(acts[l])[1](zs[l], ys[l + 1])
        out["dW%d" % l] = float((np.abs(ys[l]).T @ np.abs(g)).max())
        out["db%d" % l] = float(np.abs(g).sum(axis=0).max())
        if l:                                                   # the kernel forms no g below layer 0
            out["g%d" % l] = float((np.abs(g) @ np.abs(w[l]).T).max())
            g = g @ w[l].T
    for name, bound in out.items():
        assert bound < EXACT, (name, bound)
    return out


def integer_case(dims, acts, B, seed, nnz=3):
    """(weights, biases, x, y), small integers stored as float32: x in {-2..2}, `nnz` entries of +-1 per weight column and
    zeros elsewhere, biases in {-1..2}, targets in {-2..2}.  `integer_exactness` holds (asserted here), and every layer's
    gradient is alive: the case would say nothing about a layer whose dW is all zeros.

    Kinks.  Integer pre-activations DO sit on the kinks of relu (0) and relu6 (0 and 6), and need not avoid them, because
    the reference and the kernel agree there, both ways: relu at 0 has derivative 0 in both (oracle_train.ACTS: y > 0;
    act_grad: x > 0, asked with x = y), and relu6 at 0 and at 6 follows `y > 0 && y < 6` in both (ACTS64 above;
    train_act_grad)."""
    rng = np.random.default_rng(seed)
    ws, bs = [], []
    for i, o in zip(dims[:-1], dims[1:]):
        k = min(i, nnz)
        rows = np.argsort(rng.random((i, o)), axis=0)[:k]       # k distinct rows per column
        w = np.zeros((i, o), F)
        w[rows, np.arange(o)[None, :]] = rng.choice(np.array([-1.0, 1.0], F), size=(k, o))
        ws.append(w)
        bs.append(rng.integers(-1, 3, size=(o,)).astype(F))
    x = rng.integers(-2, 3, size=(B, dims[0])).astype(F)
    y = rng.integers(-2, 3, size=(B, dims[-1])).astype(F)
    integer_exactness(ws, bs, acts, x, y)
    _, gw, gb = mse_and_grads(ws, bs, list(acts), x, y)
    assert all(np.count_nonzero(g) for g in gw + gb), [int(np.count_nonzero(g)) for g in gw + gb]
    return ws, bs, x, y


# ---- saturated activations --------------------------------------------------------------------------------------------
# the piecewise codes and where their branches meet
SAT_DIMS, SAT_ROWS = (6, 24, 24, 3), 64
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0), "leaky_relu": (0.0,), "elu": (0.0,), "selu": (0.0,), "hard_sigmoid": (-2.5, 2.5)}
SAT_SEED, SAT_SEED_OF = 203, {"exponential": 204}             # seeds at which both conditions of `saturating_case` hold


def saturating_case(act, seed):
    """(weights, biases, acts, x, y) on (6, 24, 24, 3), `act` on both hidden layers, linear output, 64 rows: hidden biases
    uniform over +-8 (+-3.2 for `exponential`) and the first kernel scaled so that x W_0 adds a spread of about 1.5, so the
    reference's hidden pre-activations span roughly +-9 (+-4).  W_1 is scaled down where the first layer's outputs are large,
    so the second hidden layer keeps that span.  Asserted on the float64 reference alone:
      coverage   piecewise codes: every branch holds >= 10 % of the hidden pre-activations; smooth codes: >= 10 % lie
                 beyond |x| > 4 on each side (`exponential`: beyond 2, its span being +-4, and the reference is finite);
      kinks      no hidden pre-activation within 1e-3 of a kink (0; 6 for relu6; +-2.5 for hard_sigmoid).  1e-3 is three
                 orders above the float32 forward error of an O(10) sum of 24 terms: float32 and float64 take the same
                 branch everywhere, and the comparison needs no exclusions."""
    half = 4.0 if act == "exponential" else 9.0
    rng = np.random.default_rng(seed)
    ws, bs = params(SAT_DIMS, seed)
    x, y = dataset(SAT_ROWS, SAT_DIMS[0], SAT_DIMS[-1], seed + 1, offset=0.5)
    spread = half / 6.0
    bs[0] = rng.uniform(-(half - 1.0) * 0.95, (half - 1.0) * 0.95, size=bs[0].shape).astype(F)
    bs[1] = rng.uniform(-(half - 1.0) * 0.95, (half - 1.0) * 0.95, size=bs[1].shape).astype(F)
    ws[0] = (ws[0] * (spread / np.std(x.astype(np.float64) @ ws[0].astype(np.float64)))).astype(F)
    acts = (act, act, None)
    y1 = _act(act)[0](x.astype(np.float64) @ ws[0].astype(np.float64) + bs[0])
    ws[1] = (ws[1] * min(1.0, spread / np.std(y1 @ ws[1].astype(np.float64)))).astype(F)
    ys, zs = forward(ws, bs, acts, x)
    z = np.concatenate([zs[0].ravel(), zs[1].ravel()])
    assert np.all(np.isfinite(ys[-1]))
    if act in KINKS:
        edges = (-np.inf,) + KINKS[act] + (np.inf,)
        for lo, hi in zip(edges[:-1], edges[1:]):
            assert np.mean((z > lo) & (z < hi)) >= 0.10, (act, seed, lo, hi)
        for k in KINKS[act]:
            assert np.min(np.abs(z - k)) >= 1e-3, (act, seed, k)
    else:
        far = 2.0 if act == "exponential" else 4.0
        assert np.mean(z > far) >= 0.10 and np.mean(z < -far) >= 0.10, (act, seed)
    assert np.max(np.abs(z)) <= 1.5 * half, (act, seed, float(np.max(np.abs(z))))
    return ws, bs, acts, x, y
