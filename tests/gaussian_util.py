"""NumPy statement of the particle evaluator with learned-variance (Gaussian) heads (include/bbmpc.h:
bbmpc_set_mlp_logvar_head) for the tests, on tests/particle_util.py and tests/ensemble_util.py: the particle recurrence
with one term changed,

    nxt = predict_next_state_member(s_t, a_t) + (sigma + sd(s_t, a_t)) * eps[a, p, t, :]
    z = h W_v + b_v;  lv1 = max_lv - softplus(max_lv - z);  lv = min_lv + softplus(lv1 - min_lv);  sd = tstd * exp(lv / 2)

in float32 (one rounding per op), where z comes from a second oracle MLP -- the mean network with its last layer replaced by
the head -- on Handler.process_input(s, a), softplus(x) = max(x, 0) + log(1 + exp(-|x|)) as csrc/activations.hpp defines it
and tstd = std_targets + 1e-7 (1 when not normalised).  `sd64` is the float64 twin of `sd32`."""
import numpy as np

from oracle import oracle_np as O
from tests import particle_util as PU

F = np.float32


def softplus32(x):
    x = O.f32(x)
    t = O.exp32(-np.abs(x))
    return (np.maximum(x, F(0)) + O.log32((F(1) + t).astype(F))).astype(F)


def softplus64(x):
    x = np.asarray(x, np.float64)
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


class Head:
    """The log-variance head (W_v, b_v, min_lv, max_lv) of the model behind oracle Evaluator `ev`."""

    def __init__(self, ev, w_v, b_v, min_lv, max_lv):
        net, self.handler = ev.handler.dynamics, ev.handler
        S = net.weights[-1].shape[1]
        # the mean network with the head as its last layer (no activation), same class: same hidden arithmetic
        self.net = type(net)(net.weights[:-1] + [O.f32(w_v)], net.biases[:-1] + [O.f32(b_v)], net.acts[:-1] + [None])
        self.min_lv = np.broadcast_to(O.f32(min_lv), (S,)).astype(F)
        self.max_lv = np.broadcast_to(O.f32(max_lv), (S,)).astype(F)
        normd = (not self.handler.true_model) and self.handler.is_normalized
        self.tstd = (self.handler.std_t + F(1e-7)).astype(F) if normd else np.ones((S,), F)

    def z(self, s, a):
        return self.net(self.handler.process_input(s, a))

    def sd32(self, s, a):
        z = self.z(s, a)
        lv1 = (self.max_lv - softplus32((self.max_lv - z).astype(F))).astype(F)
        lv = (self.min_lv + softplus32((lv1 - self.min_lv).astype(F))).astype(F)
        return (self.tstd * O.exp32((F(0.5) * lv).astype(F))).astype(F)

    def sd64(self, s, a):
        z = self.z(s, a).astype(np.float64)
        lo, hi = self.min_lv.astype(np.float64), self.max_lv.astype(np.float64)
        lv = lo + softplus64(hi - softplus64(hi - z) - lo)
        return self.tstd.astype(np.float64) * np.exp(0.5 * lv)


def gaussian_returns_one_model(ev, head, current_states, action_sequences, eps, sigma, P, keep_states=False):
    """particle_util.particle_returns with sigma + head.sd32(s_t, a_t) as the noise scale: float32 [N, P, A]."""
    seq = O.f32(action_sequences)
    n, a, h, u = seq.shape
    state, rows, e = PU.particle_rows(O.f32(current_states), seq, O.f32(eps), P)
    sigma = O.f32(sigma)
    total = np.zeros((n * P * a,), F)
    visited = [state]
    for t in range(h):
        nxt = ev.predict_next_state(state, rows[t])
        scale = (sigma + head.sd32(state, rows[t])).astype(F)
        nxt = (nxt + (scale * e[t]).astype(F)).astype(F)
        total = (total + ev.reward(state, rows[t], nxt)).astype(F)
        state = nxt
        if keep_states:
            visited.append(state)
    total = np.where(np.isnan(total), F(-1e6), total).astype(F).reshape(n, P, a)
    return (total, visited) if keep_states else total


def gaussian_particle_returns(evs, heads, current_states, action_sequences, eps, sigma, P, keep_states=False):
    """ensemble_util.ensemble_particle_returns with head e on member e (one evaluator and one head: no ensemble): float32
    [N, P, A], on request the visited states per member."""
    E = len(evs)
    assert len(heads) == E and P % E == 0, (len(heads), E, P)
    seq = np.asarray(action_sequences)
    eps = np.asarray(eps)
    out = np.empty((seq.shape[0], P, seq.shape[1]), F)
    visited = []
    for e, (ev, head) in enumerate(zip(evs, heads)):
        r = gaussian_returns_one_model(ev, head, current_states, seq, eps[:, e::E], sigma, P // E, keep_states=keep_states)
        if keep_states:
            r, v = r
            visited.append(v)
        out[:, e::E, :] = r
    return (out, visited) if keep_states else out


class GaussianParticleEvaluator(PU.ParticleEvaluator):
    """particle_util.ParticleEvaluator over probabilistic members: reward, member 0's handler (the mean network of every
    deterministic call) and the scores from the base class, the per-particle returns from gaussian_particle_returns."""

    def __init__(self, evs, heads, num_particles, sigma, kappa, eps):
        super().__init__(evs[0].reward, evs[0].handler, num_particles, sigma, kappa, eps)
        self.evs, self.heads = list(evs), list(heads)

    def returns(self, current_states, action_sequences, it=0):
        return gaussian_particle_returns(self.evs, self.heads, current_states, action_sequences, self.eps[it], self.sigma, self.P)
