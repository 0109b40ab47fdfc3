"""Weight decay, early stopping and best-weights restore of the package's trainers: the options every
trainer and every `train(...)` takes, checked in one place, and the monitor's state machine on the host -- what
`_train_torch.DenseTrainer` runs per epoch, and the statement of what csrc/kernels_train.hpp's k_train_monitor decides on
the device.

  weight_decay   a scalar or one value per layer (finite, >= 0), on the kernels W_l only, never on biases
  decay_mode     "l2": the rule sees g + lambda_l W_l;  "decoupled" (AdamW-style): the rule runs on the data gradient g and
                 the step also subtracts lr lambda_l W_l, lr the base rate; W_l is the value before the step in both
  patience       0: no early stopping; n > 0: a fit stops after n epochs in a row without an improvement
  min_delta      v improves on the best validation loss so far if v < best - min_delta
  restore_best   at the end of the fit the parameters of the best epoch come back (weights only: the optimizer state stays)
"""
import numpy as np

DEFAULTS = dict(weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0, restore_best=False)
DECAY_MODES = ("l2", "decoupled")


def check_options(weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0, restore_best=False, n_layers=None):
    """The options as (decay float32 [n_layers] or None when every value is 0, mode, patience, min_delta, restore_best);
    ValueError for anything a trainer refuses.  A scalar decay needs `n_layers` to become a vector; without it the scalar is
    only checked."""
    if decay_mode not in DECAY_MODES:
        raise ValueError("unknown decay_mode %r: 'l2' or 'decoupled'" % (decay_mode,))
    wd = np.asarray(weight_decay, np.float64)
    if wd.ndim > 1 or not np.all(np.isfinite(wd)) or np.any(wd < 0):
        raise ValueError("weight_decay must be finite and >= 0 (a scalar or one value per layer), got %r" % (weight_decay,))
    if wd.ndim == 1 and n_layers is not None and wd.shape[0] != n_layers:
        raise ValueError("weight_decay: one value per layer (%d), got %d" % (n_layers, wd.shape[0]))
    if wd.ndim == 0 and n_layers is not None:
        wd = np.full((n_layers,), float(wd))
    if int(patience) != patience or patience < 0:
        raise ValueError("patience must be an integer >= 0 (0: no early stopping), got %r" % (patience,))
    if not np.isfinite(min_delta) or min_delta < 0:
        raise ValueError("min_delta must be finite and >= 0, got %r" % (min_delta,))
    decay = wd.astype(np.float32) if np.any(wd > 0) else None
    return decay, decay_mode, int(patience), float(min_delta), bool(restore_best)


def non_default(weight_decay=0.0, decay_mode="l2", patience=0, min_delta=0.0, restore_best=False):
    """The options that differ from DEFAULTS, checked, as keyword arguments: what a `train(...)` hands on to a trainer, so
    that a plain call reaches the trainer with the arguments it always had."""
    check_options(weight_decay, decay_mode, patience, min_delta, restore_best)
    given = dict(weight_decay=weight_decay, decay_mode=decay_mode, patience=patience, min_delta=min_delta, restore_best=restore_best)
    out = {}
    for name, value in given.items():
        same = (np.ndim(value) == 0 and value == DEFAULTS[name]) if name == "weight_decay" else value == DEFAULTS[name]
        if not same:
            out[name] = value
    return out


def monitoring(patience, restore_best):
    return patience > 0 or bool(restore_best)


def require_validation(patience, restore_best, n_val, batch_size):
    """Monitoring needs a validation loss: refuse the fit before anything runs."""
    if monitoring(patience, restore_best) and int(n_val) // int(batch_size) == 0:
        raise ValueError("early stopping / restore_best need a validation loss: %d validation rows hold no full batch of %d"
                         % (int(n_val), int(batch_size)))


class Monitor:
    """One member's state machine.  `update(k, v)` after epoch k returns (improved, stop).  The comparison is taken in
    float32, as the device takes it: v < float32(best - min_delta)."""

    def __init__(self, patience=0, min_delta=0.0):
        self.patience, self.min_delta = int(patience), np.float32(min_delta)
        self.best, self.best_epoch, self.wait, self.stopped = np.float32(np.inf), -1, 0, 0

    def update(self, k, v):
        v = np.float32(v)
        improved = bool(v < np.float32(self.best - self.min_delta))          # NaN: False
        if improved:
            self.best, self.best_epoch, self.wait = v, int(k), 0
        else:
            self.wait += 1
        if self.patience > 0 and self.wait >= self.patience:
            self.stopped = int(k) + 1
        return improved, bool(self.stopped)

    @property
    def best_val(self):
        return float(self.best) if self.best_epoch >= 0 else float("nan")
