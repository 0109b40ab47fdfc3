"""Probabilistic (Gaussian) MLP dynamics, PETS' model: a DeterministicMLP -- the MEAN network -- plus a log-variance head
(include/bbmpc.h: bbmpc_set_mlp_logvar_head).

The head is a second last Dense layer on the mean network's last hidden activation h, without an activation, in the mean's
(normalised) target space:  z = h W_v + b_v,  lv1 = max_logvar - softplus(max_logvar - z),
lv = min_logvar + softplus(lv1 - min_logvar),  var = exp(lv).  A ParticleTrajectoryEvaluator adds
(process_noise_std + std_targets * exp(lv / 2)) * eps to every predicted next state; every deterministic consumer (the
control step's record, predict_next_state, predict_trajectories, a DeterministicTrajectoryEvaluator) sees the mean network
alone.  SystemDynamicsHandler.train fits mean and head together on the Gaussian negative log-likelihood
(_train_torch.DenseTrainer, logvar_head=...).  The bounds are fixed hyper-parameters."""
import os

import numpy as np

from .. import _lib as L
from .deterministic_mlp import DeterministicMLP


def check_logvar_bounds(min_logvar, max_logvar, dim_s):
    """The bounds as float32 [dim_S] (scalars broadcast), refused as bbmpc_set_mlp_logvar_head refuses them."""
    lo = np.broadcast_to(np.asarray(min_logvar, np.float32), (dim_s,)).copy()
    hi = np.broadcast_to(np.asarray(max_logvar, np.float32), (dim_s,)).copy()
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi)) and np.all(np.abs(lo) <= L.LOGVAR_ABS_MAX)
            and np.all(np.abs(hi) <= L.LOGVAR_ABS_MAX) and np.all(lo <= hi)):
        raise ValueError("min_logvar / max_logvar must be finite, within [-%g, %g], with min_logvar <= max_logvar"
                         % (L.LOGVAR_ABS_MAX, L.LOGVAR_ABS_MAX))
    return lo, hi


def logvar_path(mlp_path):
    """`x.npz` -> `x_logvar.npz`: where the head of the model saved as `x.npz` lies."""
    mlp_path = os.fspath(mlp_path)
    return (mlp_path[:-4] if mlp_path.endswith(".npz") else mlp_path) + "_logvar.npz"


class ProbabilisticMLP(DeterministicMLP):
    def __init__(self, layers, activation_functions, min_logvar=-10.0, max_logvar=0.5, seed=None, loss_fn=None, name=None):
        super().__init__(layers, activation_functions, loss_fn=loss_fn, name=name, seed=seed)
        hidden, dim_s = self.layer_sizes[-2], self.layer_sizes[-1]
        self.min_logvar, self.max_logvar = check_logvar_bounds(min_logvar, max_logvar, dim_s)
        # Glorot-uniform / zeros like the other Dense layers, from a stream of its own: the mean network's initial weights
        # are those of DeterministicMLP(layers, activation_functions, seed=seed)
        ss = seed if isinstance(seed, np.random.SeedSequence) else np.random.SeedSequence(seed)
        rng = np.random.default_rng([int(s) for s in ss.generate_state(4)] + [1])
        lim = np.sqrt(6.0 / (hidden + dim_s))
        self.logvar_weights = rng.uniform(-lim, lim, size=(hidden, dim_s)).astype(np.float32)
        self.logvar_bias = np.zeros((dim_s,), np.float32)

    # what configure_dynamics uploads behind the model: one head
    logvar_heads = property(lambda self: [self])

    def set_logvar_head(self, weights, bias, min_logvar=None, max_logvar=None):
        w, b = np.asarray(weights, np.float32), np.asarray(bias, np.float32)
        if w.shape != self.logvar_weights.shape or b.shape != self.logvar_bias.shape:
            raise ValueError("log-variance head: kernel %s / bias %s expected" % (self.logvar_weights.shape, self.logvar_bias.shape))
        if min_logvar is not None or max_logvar is not None:
            self.min_logvar, self.max_logvar = check_logvar_bounds(self.min_logvar if min_logvar is None else min_logvar,
                                                                   self.max_logvar if max_logvar is None else max_logvar, b.shape[0])
        self.logvar_weights, self.logvar_bias = w.copy(), b.copy()
        self._version += 1

    def save(self, path):
        """The mean network as `path` (mlp.npz: it loads as a plain DeterministicMLP) and the head next to it as
        `<path without .npz>_logvar.npz`."""
        path = os.fspath(path)
        if not path.endswith(".npz"):
            path += ".npz"
        super().save(path)
        np.savez(logvar_path(path), W=self.logvar_weights, b=self.logvar_bias, min_logvar=self.min_logvar, max_logvar=self.max_logvar)

    @classmethod
    def load(cls, path):
        path = os.fspath(path)
        if not path.endswith(".npz"):
            path += ".npz"
        mean = DeterministicMLP.load(path)
        z = np.load(logvar_path(path))
        m = cls.__new__(cls)
        m.__dict__.update(mean.__dict__)
        dim_s = m.layer_sizes[-1]
        m.min_logvar, m.max_logvar = check_logvar_bounds(z["min_logvar"], z["max_logvar"], dim_s)
        m.logvar_weights = np.zeros((m.layer_sizes[-2], dim_s), np.float32)
        m.logvar_bias = np.zeros((dim_s,), np.float32)
        m.set_logvar_head(z["W"], z["b"])
        return m
