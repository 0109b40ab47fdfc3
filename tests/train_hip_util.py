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


def train(weights, biases, acts, train_in, train_out, val_in, val_out, permutations, batch_size, learning_rate=1e-3, rule="adam"):
    """oracle_train.train where it knows every activation; otherwise its loop over `mse_and_grads` above."""
    if all(a in OT.ACTS for a in acts):
        return OT.train(weights, biases, list(acts), train_in, train_out, val_in, val_out, permutations, batch_size=batch_size,
                        learning_rate=learning_rate, rule=rule)
    w = [np.array(x, np.float64) for x in weights]
    b = [np.array(x, np.float64) for x in biases]
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
