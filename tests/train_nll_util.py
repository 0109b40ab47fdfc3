"""The Gaussian-NLL rule of DenseTrainer(..., logvar_head=...) (DESIGN.md sections 8d and 8s) in float64 NumPy, on top of
train_hip_util's forward pass and oracle_train's update rules, with the regularisation of train_reg_util -- TEST
INFRASTRUCTURE ONLY.

  h = y_{L-1} (the input when L = 1);  mu = act_{L-1}(h W_{L-1} + b_{L-1});  z = h W_v + b_v
  lv1 = max_lv - softplus(max_lv - z);  lv = min_lv + softplus(lv1 - min_lv)
  loss = mean over the batch's B O elements of (mu - y)^2 exp(-lv) + lv
  d loss / d mu = 2 (mu - y) exp(-lv) / (B O)
  d loss / d z  = (1 - (mu - y)^2 exp(-lv)) sigmoid(lv1 - min_lv) sigmoid(max_lv - z) / (B O)

A head is (W_v [hidden, O], b_v [O], min_lv [O], max_lv [O]).  W_v is a kernel of the last layer for weight decay (its
lambda), b_v a bias.  Also here: the nets, heads and datasets the GPU cases of tests/test_gpu_train_hip_nll.py use, so that
tests/test_train_nll_cpu.py can check their conditions without a GPU.
"""
import numpy as np

from oracle import oracle_train as OT
from tests import train_hip_util as U
from tests import train_reg_util as RU

F = np.float32


def softplus(x):
    return np.logaddexp(0.0, x)


def sigma(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def head64(head):
    return tuple(np.asarray(a, np.float64) for a in head)


def logvar(h, head):
    """(z, lv, dlv/dz) of the head on the hidden activation h."""
    wv, bv, lo, hi = head64(head)
    z = np.asarray(h, np.float64) @ wv + bv
    lv1 = hi - softplus(hi - z)
    lv = lo + softplus(lv1 - lo)
    return z, lv, sigma(lv1 - lo) * sigma(hi - z)


def nll(ws, bs, acts, head, x, y):
    """Per-element (mu - y)^2 exp(-lv) + lv, [B, O]."""
    ys, _ = U.forward(ws, bs, acts, x)
    _, lv, _ = logvar(ys[-2], head)
    d = ys[-1] - np.asarray(y, np.float64)
    return d * d * np.exp(-lv) + lv


def nll_and_grads(ws, bs, acts, head, x, y):
    """(loss, [dW_l], [db_l], dW_v, db_v) of the batch (x, y)."""
    ys, zs = U.forward(ws, bs, acts, x)
    n = len(ws)
    _, lv, dlv = logvar(ys[n - 1], head)
    diff = ys[-1] - np.asarray(y, np.float64)
    inv = np.exp(-lv)
    wsq = diff * diff * inv
    g = 2.0 * diff * inv / diff.size
    gz = (1.0 - wsq) * dlv / diff.size
    gw, gb = [None] * n, [None] * n
    for l in reversed(range(n)):
        g = g * U._act(acts[l])[1](zs[l], ys[l + 1])
        gw[l] = ys[l].T @ g
        gb[l] = g.sum(axis=0)
        g = g @ np.asarray(ws[l], np.float64).T
        if l == n - 1:                                          # the head reads the same hidden activation
            g = g + gz @ head64(head)[0].T
    return float(np.mean(wsq + lv)), gw, gb, ys[n - 1].T @ gz, gz.sum(axis=0)


def train_nll(ws, bs, acts, head, train_in, train_out, val_in, val_out, permutations, batch_size, learning_rate=1e-3, rule="adam",
              weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0, restore_best=False):
    """oracle_train.train's loop with the head, under train_reg_util's rule (the monitor watches the validation NLL).
    Returns (w, b, (W_v, b_v), train_loss, val_loss, report); loss entries of epochs not run are NaN."""
    w = [np.array(x, np.float64) for x in ws]
    b = [np.array(x, np.float64) for x in bs]
    hv = [np.array(head[0], np.float64), np.array(head[1], np.float64)]
    lo, hi = np.asarray(head[2], np.float64), np.asarray(head[3], np.float64)
    n = len(w)
    lam = list(RU.decay_vector(weight_decay, n))
    kernels = list(range(n)) + [2 * n]                          # positions in `params` of W_0 .. W_{L-1}, W_v
    lams = lam + [lam[-1]]
    params = w + b + hv
    opt = OT.OPTIMIZERS[rule](params, learning_rate)
    epochs = len(permutations)
    tl, vl = np.full((epochs,), np.nan), np.full((epochs,), np.nan)
    monitoring = patience > 0 or restore_best
    mon, snapshot, ran = RU.Monitor(patience, min_delta), None, epochs
    for k, perm in enumerate(permutations):
        nb, acc = 0, 0.0
        for s in range(0, len(perm) - batch_size + 1, batch_size):
            idx = perm[s:s + batch_size]
            loss, gw, gb, gwv, gbv = nll_and_grads(w, b, acts, (hv[0], hv[1], lo, hi), train_in[idx], train_out[idx])
            grads = gw + gb + [gwv, gbv]
            if decay_mode == "l2":
                for i, l_ in zip(kernels, lams):
                    grads[i] = grads[i] + l_ * params[i]
                opt.step(params, grads)
            elif decay_mode == "decoupled":
                before = [params[i].copy() for i in kernels]
                opt.step(params, grads)
                for i, l_, x0 in zip(kernels, lams, before):
                    params[i] -= learning_rate * l_ * x0
            else:
                raise ValueError(decay_mode)
            acc += loss
            nb += 1
        if nb:
            tl[k] = acc / nb
        nb, acc = 0, 0.0
        for s in range(0, val_in.shape[0] - batch_size + 1, batch_size):
            acc += float(np.mean(nll(w, b, acts, (hv[0], hv[1], lo, hi), val_in[s:s + batch_size], val_out[s:s + batch_size])))
            nb += 1
        if nb:
            vl[k] = acc / nb
        if monitoring:
            assert nb, "monitoring needs a validation loss"
            if mon.update(k, vl[k]):
                snapshot = [x.copy() for x in params]
            if mon.stopped:
                ran = k + 1
                break
    if restore_best and mon.best_epoch >= 0:
        for x, s in zip(params, snapshot):
            x[...] = s
    report = dict(epochs_run=ran, best_epoch=mon.best_epoch if monitoring else -1,
                  best_val=mon.best if monitoring and mon.best_epoch >= 0 else np.nan)
    return w, b, (hv[0], hv[1]), tl, vl, report


# ---- what the GPU cases use -------------------------------------------------------------------------------------------
# one tile everywhere; ragged tiles with a swish layer below the head's input and O no multiple of 4; L = 1; the flagship
NETS = {"4-16-16-3": ((4, 16, 16, 3), ("tanh", "tanh", None)),
        "7-20-33-5": ((7, 20, 33, 5), ("swish", "tanh", None)),
        "5-3": ((5, 3), (None,)),
        "26-200-200-20": ((26, 200, 200, 20), ("tanh", "tanh", None))}
GRAD_BATCHES = (16, 24, 40, 128)                                # 24 and 40 leave a ragged last tile
GRAD_ROWS = 160


def gauss_head(ws, bs, acts, x, seed):
    """A head for the net on the rows x: a Glorot kernel scaled so that z = h W_v + b_v has unit spread over x, small biases,
    and per-dimension bounds min_lv in [-0.5, -0.2], max_lv in [0.2, 0.5] -- inside the spread of z, so that all three regimes
    of the soft clamp (below min_lv, between, above max_lv) occur.  float32."""
    rng = np.random.default_rng(seed)
    h = U.forward(ws, bs, acts, x)[0][-2]
    hidden, out = h.shape[1], np.shape(ws[-1])[1]
    lim = np.sqrt(6.0 / (hidden + out))
    wv = rng.uniform(-lim, lim, size=(hidden, out))
    wv = wv / np.std(h @ wv)
    bv = rng.normal(0.0, 0.05, size=(out,))
    lo = rng.uniform(-0.5, -0.2, size=(out,))
    hi = rng.uniform(0.2, 0.5, size=(out,))
    return wv.astype(F), bv.astype(F), lo.astype(F), hi.astype(F)


def gradient_case(net, B):
    """(ws, bs, acts, head, x, y, idx) of the gradient case (net, B): train_hip_util's parameters and shifted dataset (see
    `dataset` there), the head above, and a batch of B of the 160 rows."""
    dims, acts = NETS[net]
    ws, bs = U.params(dims, seed=11)
    x, y = U.dataset(GRAD_ROWS, dims[0], dims[-1], seed=12, offset=0.5)
    head = gauss_head(ws, bs, acts, x, seed=14)
    idx = np.random.default_rng(13 + B).permutation(GRAD_ROWS)[:B]
    return ws, bs, acts, head, x, y, idx


def clamp_shares(ws, bs, acts, head, x):
    """The shares of z above max_lv and below min_lv on the rows x."""
    h = U.forward(ws, bs, acts, x)[0][-2]
    z, _, _ = logvar(h, head)
    return float(np.mean(z > np.asarray(head[3], np.float64))), float(np.mean(z < np.asarray(head[2], np.float64)))


FIT_NETS = ("4-16-16-3", "7-20-33-5")
FIT_RULES = (("adam", 2e-3), ("sgd", 1e-2), ("rmsprop", 1e-3))
FIT_EPOCHS, FIT_TRAIN, FIT_VAL, FIT_BATCH = 3, 200, 72, 24


def fit_case(net, seed, n_val=FIT_VAL, epochs=FIT_EPOCHS):
    """(ws, bs, acts, head, tin, tout, vin, vout, perms) of a whole-fit case; net: a name in NETS, or (dims, acts)."""
    dims, acts = NETS[net] if isinstance(net, str) else net
    ws, bs = U.params(dims, seed=seed)
    x, y = U.dataset(FIT_TRAIN + n_val, dims[0], dims[-1], seed=seed + 1)
    head = gauss_head(ws, bs, acts, x, seed=seed + 3)
    rng = np.random.default_rng(seed + 2)
    perms = [rng.permutation(FIT_TRAIN) for _ in range(epochs)]
    return ws, bs, acts, head, x[:FIT_TRAIN], y[:FIT_TRAIN], x[FIT_TRAIN:], y[FIT_TRAIN:], perms


def rising_case(seed=300):
    """`fit_case("4-16-16-3")` whose validation targets are the NEGATED function of the inputs: the closer the mean network
    comes to the training targets, the further it is from these.  With sgd at 5e-2 the validation NLL is lowest after the
    first epoch and rises from there (checked in tests/test_train_nll_cpu.py on the float64 rule, with a margin far above
    float32's error), so patience = 1 stops after the second epoch and restores the first one's parameters."""
    ws, bs, acts, head, tin, tout, vin, vout, perms = fit_case("4-16-16-3", seed, epochs=4)
    return ws, bs, acts, head, tin, tout, vin, (-vout).astype(F), perms


RISING = dict(rule="sgd", learning_rate=5e-2, patience=1, restore_best=True)
