"""Bootstrap ensemble of DeterministicMLPs for PETS-style trajectory sampling (include/bbmpc.h: bbmpc_set_mlp_ensemble).

`num_members` networks of one shape with distinct initial weights.  SystemDynamicsHandler.train fits each on its own
bootstrap resample of the training rows; a ParticleTrajectoryEvaluator then rolls particle p of every candidate through
member p % num_members for the whole horizon, so member disagreement shows as spread of the per-particle returns.
To every deterministic consumer (the control step's record, predict_next_state, predict_trajectories, a
DeterministicTrajectoryEvaluator) the ensemble IS its member 0: `weights`, `biases`, `activation_codes` and `__call__`
are that member's.

With `probabilistic=True` the members are ProbabilisticMLPs (PETS' probabilistic ensemble): each carries a log-variance
head on bounds the members share, uploaded behind the members (bbmpc_set_mlp_logvar_head)."""
import os

import numpy as np

from .. import _lib as L
from .deterministic_mlp import DeterministicMLP
from .probabilistic_mlp import ProbabilisticMLP, logvar_path


def _member_paths(path):
    """(directory, member 0's file): `path` is the directory, or the `mlp.npz` inside it (what SystemDynamicsHandler passes)."""
    path = os.fspath(path)
    if path.endswith(".npz"):
        return os.path.dirname(path) or ".", path
    return path, os.path.join(path, "mlp.npz")


class EnsembleMLP:
    _bbmpc_dynamics_kind = L.DYN_MLP

    def __init__(self, layers, activation_functions, num_members, seed=None, loss_fn=None, name=None, probabilistic=False,
                 min_logvar=-10.0, max_logvar=0.5):
        e = int(num_members)
        if not 1 <= e <= L.MAX_ENSEMBLE_MEMBERS:
            raise ValueError("num_members must be in [1, %d], got %r" % (L.MAX_ENSEMBLE_MEMBERS, num_members))
        self.name = name
        # one child seed per member: distinct initial weights, reproducible from `seed`
        children = np.random.SeedSequence(seed).spawn(e)
        if probabilistic:
            self.members = [ProbabilisticMLP(layers, activation_functions, min_logvar=min_logvar, max_logvar=max_logvar,
                                             seed=child, loss_fn=loss_fn, name=name) for child in children]
        else:
            self.members = [DeterministicMLP(layers, activation_functions, loss_fn=loss_fn, name=name, seed=child)
                            for child in children]

    @classmethod
    def from_members(cls, members):
        members = list(members)
        if not 1 <= len(members) <= L.MAX_ENSEMBLE_MEMBERS:
            raise ValueError("1..%d members expected, got %d" % (L.MAX_ENSEMBLE_MEMBERS, len(members)))
        for m in members[1:]:
            if m.layer_sizes != members[0].layer_sizes or m.activation_codes != members[0].activation_codes:
                raise ValueError("the members of an ensemble share layer sizes and activations")
        heads = [isinstance(m, ProbabilisticMLP) for m in members]
        if any(heads) and not all(heads):
            raise ValueError("the members of an ensemble are either all ProbabilisticMLP or all plain DeterministicMLP")
        for m in members[1:]:
            if heads[0] and not (np.array_equal(m.min_logvar, members[0].min_logvar) and
                                 np.array_equal(m.max_logvar, members[0].max_logvar)):
                raise ValueError("the members of a probabilistic ensemble share min_logvar / max_logvar")
        self = cls.__new__(cls)
        self.name = members[0].name
        self.members = members
        return self

    num_members = property(lambda self: len(self.members))
    # member 0 is the model of every deterministic consumer
    layer_sizes = property(lambda self: self.members[0].layer_sizes)
    activation_codes = property(lambda self: self.members[0].activation_codes)
    weights = property(lambda self: self.members[0].weights)
    biases = property(lambda self: self.members[0].biases)
    loss_fn = property(lambda self: self.members[0].loss_fn)
    probabilistic = property(lambda self: isinstance(self.members[0], ProbabilisticMLP))
    # what configure_dynamics uploads behind the members: head e belongs to member e (none for plain members)
    logvar_heads = property(lambda self: list(self.members) if self.probabilistic else [])
    min_logvar = property(lambda self: self.members[0].min_logvar)
    max_logvar = property(lambda self: self.members[0].max_logvar)
    # bumped by any member's set_weights: evaluators re-upload the model and the members
    _version = property(lambda self: sum(m._version for m in self.members))

    def set_weights(self, weights, biases):
        """Member 0's (the DeterministicMLP interface); the others through `members[i].set_weights`."""
        self.members[0].set_weights(weights, biases)

    def __call__(self, x, train=False):
        return self.members[0](x, train)

    def get_loss(self, expected_output, predictions):
        return self.members[0].get_loss(expected_output, predictions)

    def get_validation_loss(self, expected_output, predictions):
        return self.members[0].get_validation_loss(expected_output, predictions)

    def save(self, path):
        """Member 0 as `mlp.npz` -- the directory also loads as a plain DeterministicMLP -- and member i >= 1 as
        `mlp_member{i}.npz` next to it; a probabilistic member's head as `mlp_logvar.npz` / `mlp_member{i}_logvar.npz`."""
        folder, first = _member_paths(path)
        os.makedirs(folder, exist_ok=True)
        self.members[0].save(first)
        for i, m in enumerate(self.members[1:], start=1):
            m.save(os.path.join(folder, "mlp_member%d.npz" % i))
        i = len(self.members)
        while os.path.exists(os.path.join(folder, "mlp_member%d.npz" % i)):       # a larger ensemble saved here before
            os.remove(os.path.join(folder, "mlp_member%d.npz" % i))
            i += 1
        # heads saved here before that no longer belong to a member
        files = [first] + [os.path.join(folder, "mlp_member%d.npz" % j) for j in range(1, i)]
        for j, f in enumerate(files):
            if not (self.probabilistic and j < len(self.members)) and os.path.exists(logvar_path(f)):
                os.remove(logvar_path(f))

    @classmethod
    def load(cls, path):
        folder, first = _member_paths(path)
        kind = ProbabilisticMLP if os.path.exists(logvar_path(first)) else DeterministicMLP
        members = [kind.load(first)]
        while os.path.exists(os.path.join(folder, "mlp_member%d.npz" % len(members))):
            members.append(kind.load(os.path.join(folder, "mlp_member%d.npz" % len(members))))
        return cls.from_members(members)
