"""NumPy statement of the particle trajectory evaluator (include/bbmpc.h: bbmpc_set_particles) for the tests: the
oracle's Evaluator with the recurrence

    nxt = predict_next_state(s_t, a_t) + sigma * eps[a, p, t, :]      R += reward(s_t, a_t, nxt)      s_{t+1} = nxt
    r[n, p, a] = R (NaN -> -1e6);   mean = (sum_p r) / P;   var = (sum_p (r - mean)^2) / P;   score = mean - kappa sqrt(var)

in float32 (one rounding per op, sums in index order) and a float64 twin.  The oracle's CEM / PI2 / RandomSearch take a
ParticleEvaluator as their `evaluator` unchanged; it keeps an iteration counter to pick eps[it]."""
import numpy as np

from oracle import oracle_np as O
from tests import philox_np as PH
from tests.parity_util import CHEETAH_INDICATORS
from tests.traj_util import pendulum_reward64, pendulum_step64

F = np.float32
NOISE_PROCESS = 11


def particle_rows(current_states, action_sequences, eps, P):
    """Rows b = (n * P + p) * A + a: (start states [B,S], actions [H,B,U], noise [H,B,S])."""
    seq = np.asarray(action_sequences)
    n, a, h, u = seq.shape
    eps = np.asarray(eps)
    assert eps.shape[:3] == (a, P, h), (eps.shape, (a, P, h))
    rows = np.repeat(seq[:, None], P, axis=1).reshape(n * P * a, h, u).transpose(1, 0, 2)
    state = np.tile(np.asarray(current_states), (n * P, 1))
    e = np.tile(eps.transpose(1, 0, 2, 3).reshape(P * a, h, -1), (n, 1, 1)).transpose(1, 0, 2)
    return state, rows, e


def particle_returns(ev, current_states, action_sequences, eps, sigma, P, keep_states=False):
    """float32 per-particle returns [N, P, A] of oracle Evaluator `ev` (and the visited states [H+1][B,S] on request)."""
    seq = O.f32(action_sequences)
    n, a, h, u = seq.shape
    state, rows, e = particle_rows(O.f32(current_states), seq, O.f32(eps), P)
    sigma = O.f32(sigma)
    total = np.zeros((n * P * a,), F)
    visited = [state]
    for t in range(h):
        nxt = ev.predict_next_state(state, rows[t])
        nxt = (nxt + (sigma * e[t]).astype(F)).astype(F)
        total = (total + ev.reward(state, rows[t], nxt)).astype(F)
        state = nxt
        if keep_states:
            visited.append(state)
    total = np.where(np.isnan(total), F(-1e6), total).astype(F).reshape(n, P, a)
    return (total, visited) if keep_states else total


def pendulum_particle_returns64(current_states, action_sequences, eps, sigma, P, as_executed=True):
    """The same recurrence for the analytic pendulum in float64: [N, P, A]."""
    seq = np.asarray(action_sequences, np.float64)
    n, a, h, u = seq.shape
    state, rows, e = particle_rows(np.asarray(current_states, np.float64), seq, np.asarray(eps, np.float64), P)
    sigma = np.asarray(sigma, np.float64)
    total = np.zeros((n * P * a,))
    for t in range(h):
        nxt = pendulum_step64(state, rows[t]) + sigma * e[t]
        total = total + pendulum_reward64(state, nxt, rows[t], as_executed)
        state = nxt
    return np.where(np.isnan(total), -1e6, total).reshape(n, P, a)


def aggregate32(returns, kappa):
    """[N, P, A] -> scores [N, A] in float32, sums over p in index order; kappa == 0: the sqrt term is not evaluated."""
    r = O.f32(returns)
    P = r.shape[1]
    mean = (O.seq_sum(r, axis=1) / F(P)).astype(F)
    if kappa == 0:
        return mean
    d = (r - mean[:, None]).astype(F)
    var = (O.seq_sum((d * d).astype(F), axis=1) / F(P)).astype(F)
    return (mean - (F(kappa) * O.sqrt32(var)).astype(F)).astype(F)


def aggregate64(returns, kappa):
    r = np.asarray(returns, np.float64)
    return r.mean(axis=1) - kappa * r.std(axis=1)


def aggregate_bound(returns, kappa):
    """|score32 - score64| <= 64 P 2^-24 (1 + kappa) max_p |r_p|  per (n, a): a P-term sum carries at most P ulp-level
    errors of the running sum, the variance the same again, and d sqrt(v) ~ dv / (2 sqrt(v)) -- which is why the bound is
    asserted only where the float64 std is at least 1 % of max_p |r_p| (`rows`)."""
    r = np.asarray(returns, np.float64)
    big = np.abs(r).max(axis=1)
    rows = r.std(axis=1) >= 0.01 * big
    return 64.0 * r.shape[1] * 2.0 ** -24 * (1.0 + kappa) * big, rows


class ParticleEvaluator(O.Evaluator):
    """oracle_np.Evaluator whose __call__ returns the particle scores.  eps: [A,P,H,S], or [iters][A,P,H,S] consumed one
    per call (the optimizers call the evaluator once per iteration; `it` wraps so that a control step can be repeated)."""

    def __init__(self, reward, handler, num_particles, sigma, kappa, eps):
        super().__init__(reward, handler)
        self.P, self.sigma, self.kappa = int(num_particles), O.f32(sigma), float(kappa)
        eps = O.f32(eps)
        self.eps = eps[None] if eps.ndim == 4 else eps
        self.it = 0
        self.last_returns = None

    def returns(self, current_states, action_sequences, it=0):
        return particle_returns(self, current_states, action_sequences, self.eps[it], self.sigma, self.P)

    def __call__(self, current_states, action_sequences, return_final_state=False):
        assert not return_final_state
        self.last_returns = self.returns(current_states, action_sequences, self.it % self.eps.shape[0])
        self.it += 1
        return aggregate32(self.last_returns, self.kappa)


def cheetah_noisy_margin(visited):
    """parity_util.cheetah_threshold_margin on the NOISY trajectories: visited [H+1][B,S] -> [B] float64."""
    margin = np.full((visited[0].shape[0],), np.inf)
    for t, state in enumerate(visited[:-1]):
        for i, thr in CHEETAH_INDICATORS:
            margin = np.minimum(margin, np.abs(state[:, i].astype(np.float64) - thr) / (t + 1))
    return margin


def process_noise_np(seed, control_step, iteration, A, P, H, S, agent_offset=0):
    """The documented generator: counter (p, ga * Qp + (j >> 2), control_step, (11 << 16) | iter), j = t * S + s,
    Qp = ceil(H S / 4); element j from word j & 3, Box-Muller on the word pairs (0,1), (2,3).  float64 [A,P,H,S]."""
    hs = H * S
    hs4 = (hs + 3) // 4 * 4                             # whole Philox blocks (Qp is the same): a ragged last block's
    w = PH.words(seed, control_step, NOISE_PROCESS, iteration, P, A, hs4, agent_offset=agent_offset)     # [P, A, hs4]
    u = ((w >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23                     # elements still pair with its words
    q = u.reshape(P, A, -1, 2, 2)                      # [.., block, pair, (u1, u2)]
    r = np.sqrt(-2.0 * np.log(q[..., 0]))
    ang = 2.0 * np.pi * q[..., 1]
    z = np.stack([r * np.cos(ang), r * np.sin(ang)], axis=-1).reshape(P, A, -1)[:, :, :hs]
    return z.transpose(1, 0, 2).reshape(A, P, H, S)
