"""NumPy statement of trajectory sampling through a model ensemble (include/bbmpc.h: bbmpc_set_mlp_ensemble) for the
tests, built from tests/particle_util.py alone: particle p of every candidate and agent follows member p % E for the
whole horizon, everything else is the particle evaluator's recurrence -- so the returns of member e's particles are
particle_util.particle_returns of that member's evaluator on the noise paths e, e + E, ..."""
import numpy as np

from tests import particle_util as PU

F = np.float32


def ensemble_particle_returns(evs, current_states, action_sequences, eps, sigma, P, keep_states=False):
    """float32 per-particle returns [N, P, A] of the oracle Evaluators `evs` (one per member); on request also the visited
    states per member, [E] lists of [H+1][N * P/E * A, S] in particle_util's row order."""
    E = len(evs)
    assert P % E == 0, (P, E)
    seq = np.asarray(action_sequences)
    eps = np.asarray(eps)
    out = np.empty((seq.shape[0], P, seq.shape[1]), F)
    visited = []
    for e, ev in enumerate(evs):
        r = PU.particle_returns(ev, current_states, seq, eps[:, e::E], sigma, P // E, keep_states=keep_states)
        if keep_states:
            r, v = r
            visited.append(v)
        out[:, e::E, :] = r
    return (out, visited) if keep_states else out


class EnsembleParticleEvaluator(PU.ParticleEvaluator):
    """particle_util.ParticleEvaluator over the members' evaluators: the reward, the handler of member 0 (the model of
    every deterministic call, predict_next_state included) and the scores come from the base class, the per-particle
    returns from ensemble_particle_returns."""

    def __init__(self, evs, num_particles, sigma, kappa, eps):
        super().__init__(evs[0].reward, evs[0].handler, num_particles, sigma, kappa, eps)
        self.evs = list(evs)

    def returns(self, current_states, action_sequences, it=0):
        return ensemble_particle_returns(self.evs, current_states, action_sequences, self.eps[it], self.sigma, self.P)
