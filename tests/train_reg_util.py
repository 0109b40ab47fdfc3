"""The rule of DESIGN.md section 8r -- weight decay, early stopping, best-weights restore -- stated once, in float64, on top
of oracle_train's forward / backward / Keras update rules.  TEST INFRASTRUCTURE ONLY.

Weight decay (kernels W_l only, never biases; lambda_l per layer; W_l the value BEFORE the step):
  "l2"         the update rule sees g_W + lambda_l W_l, then runs as it always does
  "decoupled"  the rule runs on the data gradient alone; the step then also subtracts lr lambda_l W_l, lr the base rate
Monitoring, after every epoch k with validation loss v_k:
  v_k improves if v_k < best - min_delta (best starts at +inf; NaN never improves)
  improvement: best = v_k, best_epoch = k, wait = 0, the parameters are copied to a snapshot;  otherwise: wait += 1
  patience > 0 and wait >= patience: stop after epoch k; the losses of the epochs not run are NaN
  at the end, with restore_best and best_epoch >= 0: the parameters become the snapshot (the optimizer state stays)
Reported losses are the data term (MSE).
"""
import numpy as np

from oracle import oracle_train as OT
from tests import train_hip_util as U


def decay_vector(weight_decay, n_layers):
    wd = np.asarray(weight_decay, np.float64)
    return np.full((n_layers,), float(wd)) if wd.ndim == 0 else wd


def decayed_step(opt, w, b, gw, gb, lr, weight_decay, mode):
    """One update of (w, b), in place, from the data gradients (gw, gb) under `opt` (an oracle_train optimizer)."""
    lam = decay_vector(weight_decay, len(w))
    if mode == "l2":
        opt.step(w + b, [g + l * x for g, l, x in zip(gw, lam, w)] + list(gb))
    elif mode == "decoupled":
        before = [x.copy() for x in w]
        opt.step(w + b, list(gw) + list(gb))
        for x, l, x0 in zip(w, lam, before):
            x -= lr * l * x0
    else:
        raise ValueError(mode)


class Monitor:
    def __init__(self, patience, min_delta):
        self.patience, self.min_delta = patience, min_delta
        self.best, self.best_epoch, self.wait, self.stopped = np.inf, -1, 0, False

    def update(self, k, v):
        """-> improved"""
        improved = bool(v < self.best - self.min_delta)
        if improved:
            self.best, self.best_epoch, self.wait = v, k, 0
        else:
            self.wait += 1
        if self.patience > 0 and self.wait >= self.patience:
            self.stopped = True
        return improved


def monitor_sequence(vals, patience, min_delta):
    """The state machine on an injected loss sequence: (epochs_run, best_epoch, best_val, improved flags of the epochs run)."""
    mon, flags = Monitor(patience, min_delta), []
    for k, v in enumerate(vals):
        flags.append(mon.update(k, v))
        if mon.stopped:
            break
    return len(flags), mon.best_epoch, (mon.best if mon.best_epoch >= 0 else np.nan), flags


def train(weights, biases, acts, train_in, train_out, val_in, val_out, permutations, batch_size, learning_rate=1e-3, rule="adam",
          weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0, restore_best=False, opt=None):
    """train_hip_util.train's loop under the rule above.  Returns (w, b, train_loss, val_loss, report) with report =
    dict(epochs_run, best_epoch, best_val); loss entries of epochs not run are NaN."""
    w = [np.array(x, np.float64) for x in weights]
    b = [np.array(x, np.float64) for x in biases]
    if opt is None:
        opt = OT.OPTIMIZERS[rule](w + b, learning_rate)
    epochs = len(permutations)
    tl, vl = np.full((epochs,), np.nan), np.full((epochs,), np.nan)
    monitoring = patience > 0 or restore_best
    mon, snapshot, ran = Monitor(patience, min_delta), None, epochs
    for k, perm in enumerate(permutations):
        nb, acc = 0, 0.0
        for s in range(0, len(perm) - batch_size + 1, batch_size):
            idx = perm[s:s + batch_size]
            loss, gw, gb = U.mse_and_grads(w, b, acts, train_in[idx], train_out[idx])
            decayed_step(opt, w, b, gw, gb, learning_rate, weight_decay, decay_mode)
            acc += loss
            nb += 1
        if nb:
            tl[k] = acc / nb
        nb, acc = 0, 0.0
        for s in range(0, val_in.shape[0] - batch_size + 1, batch_size):
            d = U.forward(w, b, acts, val_in[s:s + batch_size])[0][-1] - val_out[s:s + batch_size]
            acc += float(np.mean(d * d))
            nb += 1
        if nb:
            vl[k] = acc / nb
        if monitoring:
            assert nb, "monitoring needs a validation loss"
            if mon.update(k, vl[k]):
                snapshot = [x.copy() for x in w + b]
            if mon.stopped:
                ran = k + 1
                break
    if restore_best and mon.best_epoch >= 0:
        for x, s in zip(w + b, snapshot):
            x[...] = s
    report = dict(epochs_run=ran, best_epoch=mon.best_epoch if monitoring else -1,
                  best_val=mon.best if monitoring and mon.best_epoch >= 0 else np.nan)
    return w, b, tl, vl, report


def shrink_f32(w, lr, lam, steps):
    """A kernel under `steps` SGD steps of "l2" decay with a zero data gradient, in float32 in the kernel's order of
    operations: g' = fma(lam, w, 0) = lam w;  w = w + (-lr) g'.  With lr and lam powers of two both products are exact and
    each step rounds once -- to the nearest float32 of w (1 - lr lam) -- whether or not the compiler contracts the
    multiply-add."""
    w = np.asarray(w, np.float32).copy()
    lr, lam = np.float32(lr), np.float32(lam)
    for _ in range(steps):
        g = (lam * w).astype(np.float32)
        w = (w + (-lr) * g).astype(np.float32)
    return w
