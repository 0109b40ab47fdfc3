"""Plan gradients (bbmpc_plan_gradient): the NumPy statement of the return and of its gradient in the
actions, the activation-derivative table and the test networks that tests/test_plan_gradient_cpu.py (statement against
autograd and finite differences) and tests/test_gpu_plan_gradient.py (device against statement) share.  Test infrastructure only.

The statement.  Learned dynamics (W_l, b_l, act_l; statistics mean_s, std_s, mean_a, std_a, mean_t, std_t or none), a reward
network (tests/reward_mlp_util.Net's fields: input_mask, statistics), optionally a value network with weight w.  For row b,
s_0 = states[b], a_t = seq[b, t]:
    x       = concat(s_t, a_t);  x = (x - mean_in) / (std_in + float32(1e-7))        (skipped without statistics)
    y       = DynStack(x);       s_{t+1} = s_t + mean_t + y * (std_t + float32(1e-7))  (s_t + y without statistics)
    r_t     = RewardMLP(s_t, a_t, s_{t+1})                                           (reward_mlp_util's rule)
    R[b]    = sum over t ascending of r_t  +  w * V(s_Hq)                            (no NaN rule, no clip, no penalty)
    G[b,t,u] = dR[b] / da_t[u]
by reverse accumulation with lambda_t = dR/ds_t: lambda_Hq = w * grad V; at step t first lambda_{t+1} += dr_t/ds_{t+1}, then
G_t = dr_t/da_t + J_a^T lambda_{t+1} and lambda_t = dr_t/ds_t + lambda_{t+1} + J_s^T lambda_{t+1}.

Kinks.  relu, relu6, leaky_relu and hard_sigmoid are piecewise linear (selu's slope jumps at 0 as well).  At a kink the
derivative is the slope of the branch the forward comparison takes: relu x > 0 ? 1 : 0; relu6 0 for x < 0 and x > 6, else 1;
leaky_relu x > 0 ? 1 : 0.2; hard_sigmoid (t = 0.2 x + 0.5) 0 for t < 0 and t > 1, else 0.2; selu x > 0 ? lambda : lambda
alpha e^x -- csrc/activations_grad.hpp states the same table.  value_and_grad's info['margin'] reports how far the pre-activations of a
computation stay from those points, so tests that compare against autograd or across precisions can insist on a distance.

Every function takes dt: np.float64 is the statement, np.float32 the same operations in single precision (the yardstick of
the GPU test's tolerance)."""
import numpy as np

F = np.float32
ACT_NAMES = [None, "tanh", "relu", "sigmoid", "elu", "selu", "softplus", "softsign", "exponential", "hard_sigmoid", "swish",
             "leaky_relu", "relu6"]
ACT = {n: i for i, n in enumerate(ACT_NAMES)}                 # the BBMPC_ACT_* codes
SELU_L, SELU_LA = 1.0507009873554805, 1.7580993408473766      # lambda, lambda * alpha
KINKS = {"relu": (0.0,), "relu6": (0.0, 6.0), "leaky_relu": (0.0,), "hard_sigmoid": (-2.5, 2.5), "selu": (0.0,)}


def act_value_grad(name, x):
    """(act(x), act'(x)) elementwise, in x's dtype"""
    one = x.dtype.type(1)
    if name is None:
        return x, np.ones_like(x)
    if name == "tanh":
        y = np.tanh(x)
        return y, one - y * y
    if name == "relu":
        return np.maximum(x, 0), (x > 0).astype(x.dtype)
    if name == "sigmoid":
        y = one / (one + np.exp(-x))
        return y, y * (one - y)
    if name == "elu":
        e = np.exp(np.minimum(x, 0))
        return np.where(x > 0, x, e - one), np.where(x > 0, one, e)
    if name == "selu":
        e = np.exp(np.minimum(x, 0))
        lam, la = x.dtype.type(SELU_L), x.dtype.type(SELU_LA)
        return np.where(x > 0, lam * x, la * e - la), np.where(x > 0, lam, la * e)
    if name == "softplus":
        return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x))), one / (one + np.exp(-x))
    if name == "softsign":
        r = one / (one + np.abs(x))
        return x * r, r * r
    if name == "exponential":
        y = np.exp(x)
        return y, y
    if name == "hard_sigmoid":
        t = x.dtype.type(0.2) * x + x.dtype.type(0.5)
        return np.clip(t, 0, 1), np.where((t < 0) | (t > 1), 0, x.dtype.type(0.2)).astype(x.dtype)
    if name == "swish":
        s = one / (one + np.exp(-x))
        return x * s, s + x * s * (one - s)
    if name == "leaky_relu":
        return np.maximum(x, x.dtype.type(0.2) * x), np.where(x > 0, one, x.dtype.type(0.2)).astype(x.dtype)
    if name == "relu6":
        return np.clip(x, 0, 6), np.where((x < 0) | (x > 6), 0, one).astype(x.dtype)
    raise AssertionError(name)


class Stack:
    """A Dense stack with tests/reward_mlp_util.Net's fields (ws, bs, acts, stats, mask, S, U, D, dims) and any of the
    twelve activations.  mask 1 | 2 | 4 selects s_t, a_t, s_{t+1}; a value network has mask 1."""

    def __init__(self, name, S, U, mask, hidden, acts, normalized, seed, out=1):
        self.name, self.S, self.U, self.mask, self.acts = name, S, U, mask, list(acts)
        self.D = (S if mask & 1 else 0) + (U if mask & 2 else 0) + (S if mask & 4 else 0)
        self.dims = [self.D] + list(hidden) + [out]
        assert len(self.acts) == len(self.dims) - 1
        rng = np.random.default_rng(seed)
        self.ws = [rng.normal(0, 1.0 / np.sqrt(k), (k, m)).astype(F) for k, m in zip(self.dims[:-1], self.dims[1:])]
        self.bs = [rng.normal(0, 0.1, (m,)).astype(F) for m in self.dims[1:]]
        self.stats = None
        if normalized:
            self.stats = [rng.normal(0, 0.2, self.D).astype(F), rng.uniform(0.5, 1.5, self.D).astype(F),
                          np.array([0.3], F), np.array([1.7], F)]

    def codes(self):
        return [ACT[a] for a in self.acts]


class Dynamics:
    """Learned dynamics over (s, a): dims S+U .. S, statistics mean_s, std_s, mean_a, std_a, mean_t, std_t or none."""

    def __init__(self, name, S, U, hidden, acts, normalized, seed):
        self.name, self.S, self.U, self.acts = name, S, U, list(acts)
        self.dims = [S + U] + list(hidden) + [S]
        assert len(self.acts) == len(self.dims) - 1
        rng = np.random.default_rng(seed)
        self.ws = [rng.normal(0, 1.0 / np.sqrt(k), (k, m)).astype(F) for k, m in zip(self.dims[:-1], self.dims[1:])]
        self.bs = [rng.normal(0, 0.1, (m,)).astype(F) for m in self.dims[1:]]
        self.stats = None
        if normalized:
            self.stats = [rng.normal(0, 0.2, S).astype(F), rng.uniform(0.5, 1.5, S).astype(F), rng.normal(0, 0.1, U).astype(F),
                          rng.uniform(0.5, 1.5, U).astype(F), rng.normal(0, 0.01, S).astype(F), rng.uniform(0.05, 0.15, S).astype(F)]
        else:                                                   # raw outputs are the state change itself: keep it small
            self.ws[-1] = (self.ws[-1] * 0.1).astype(F)
            self.bs[-1] = (self.bs[-1] * 0.1).astype(F)

    def codes(self):
        return [ACT[a] for a in self.acts]


def _eps(dt):
    return dt(F(1e-7))


def _forward(net, x, dt, margins):
    """x [B, in] (already normalised) -> (last layer's value [B, out], [act' of every layer])"""
    ds = []
    for w, b, a in zip(net.ws, net.bs, net.acts):
        z = x @ w.astype(dt) + b.astype(dt)
        for kink in KINKS.get(a, ()):
            margins.append(float(np.min(np.abs(z - kink))))
        x, d = act_value_grad(a, z)
        ds.append(d)
    return x, ds


def _backward(net, ds, g, dt):
    """g [B, out] = dR/d(last layer's value) -> dR/d(normalised input) [B, in]"""
    for w, d in zip(reversed(net.ws), reversed(ds)):
        g = (g * d) @ w.astype(dt).T
    return g


def _in_stats(net, dt):
    if net.stats is None:
        return None, None
    return net.stats[0].astype(dt), net.stats[1].astype(dt) + _eps(dt)


def _assemble(net, cur, act, nxt):
    blocks = ([cur] if net.mask & 1 else []) + ([act] if net.mask & 2 else []) + ([nxt] if net.mask & 4 else [])
    return np.concatenate(blocks, 1)


def value_and_grad(dyn, rew, val, w, states, seq, dt=np.float64, info=None):
    """states [B, S], seq [B, Hq, U] -> (R [B], G [B, Hq, U]) in dt.  val = None: no terminal term.  info (a dict) receives
    'margin', the smallest distance of a kinked activation's pre-activation from its kink (inf without one), and 'states'."""
    dt = np.dtype(dt).type
    s = np.asarray(states, dt)
    seq = np.asarray(seq, dt)
    B, Hq, U = seq.shape
    S = dyn.S
    margins = [np.inf]
    if dyn.stats is not None:
        mean_in = np.concatenate([dyn.stats[0], dyn.stats[2]]).astype(dt)
        den_in = np.concatenate([dyn.stats[1], dyn.stats[3]]).astype(dt) + _eps(dt)
        mean_t, std_t = dyn.stats[4].astype(dt), dyn.stats[5].astype(dt) + _eps(dt)
    rmean, rden = _in_stats(rew, dt)
    total = np.zeros(B, dt)
    cache, traj = [], []
    for t in range(Hq):
        a = seq[:, t]
        x = np.concatenate([s, a], 1)
        if dyn.stats is not None:
            x = (x - mean_in) / den_in
        y, dd = _forward(dyn, x, dt, margins)
        s1 = s + (mean_t + y * std_t if dyn.stats is not None else y)
        xr = _assemble(rew, s, a, s1)
        if rmean is not None:
            xr = (xr - rmean) / rden
        yr, dr = _forward(rew, xr, dt, margins)
        r = yr[:, 0] * dt(rew.stats[3][0]) + dt(rew.stats[2][0]) if rmean is not None else yr[:, 0]
        total = total + r
        cache.append((dd, dr))
        traj.append(s1)
        s = s1
    lam = np.zeros((B, S), dt)
    if val is not None:
        vmean, vden = _in_stats(val, dt)
        xv = (s - vmean) / vden if vmean is not None else s
        yv, dv = _forward(val, xv, dt, margins)
        v = yv[:, 0] * dt(val.stats[3][0]) + dt(val.stats[2][0]) if vmean is not None else yv[:, 0]
        total = total + dt(w) * v
        seed = np.full((B, 1), dt(w) * (dt(val.stats[3][0]) if vmean is not None else dt(1)), dt)
        g = _backward(val, dv, seed, dt)
        lam = g / vden if vmean is not None else g
    G = np.zeros((B, Hq, U), dt)
    for t in range(Hq - 1, -1, -1):
        dd, dr = cache[t]
        seed = np.full((B, 1), dt(rew.stats[3][0]) if rmean is not None else dt(1), dt)
        g = _backward(rew, dr, seed, dt)
        if rmean is not None:
            g = g / rden
        o = 0
        gs = np.zeros((B, S), dt)
        ga = np.zeros((B, U), dt)
        if rew.mask & 1:
            gs = g[:, o:o + S]
            o += S
        if rew.mask & 2:
            ga = g[:, o:o + U]
            o += U
        if rew.mask & 4:
            lam = lam + g[:, o:o + S]
        gx = _backward(dyn, dd, lam * std_t if dyn.stats is not None else lam, dt)
        if dyn.stats is not None:
            gx = gx / den_in
        G[:, t] = ga + gx[:, S:]
        lam = (gs + lam) + gx[:, :S]
    if info is not None:
        info["margin"] = float(min(margins))
        info["states"] = np.stack(traj, 1)
    return total, G


def inputs(dyn, rew, val, w, B, Hq, margin, base_seed=0, tries=400, scale=0.5):
    """(states [B, S], seq [B, Hq, U], seed, margin found): the first seed base_seed, base_seed + 1, ... whose float64
    pre-activations of every kinked activation stay at least `margin` from the kink."""
    for seed in range(base_seed, base_seed + tries):
        rng = np.random.default_rng(seed)
        states = rng.normal(0, scale, (B, dyn.S)).astype(F)
        seq = rng.uniform(-1, 1, (B, Hq, dyn.U)).astype(F)
        info = {}
        value_and_grad(dyn, rew, val, w, states, seq, info=info)
        if info["margin"] >= margin:
            return states, seq, seed, info["margin"]
    raise AssertionError("no seed in [%d, %d) keeps the pre-activations %g away from the kinks" % (base_seed, base_seed + tries, margin))


def row_gap(G, G_ref):
    """largest |G - G_ref| of a row over the row's largest |G_ref| -> [B]"""
    B = G.shape[0]
    num = np.max(np.abs(np.asarray(G, np.float64) - G_ref).reshape(B, -1), 1)
    return num / np.maximum(np.max(np.abs(G_ref).reshape(B, -1), 1), 1e-30)


# ---- the CPU test's networks: S = 3, U = 2, every activation, every mask, normalised and raw ------------------------------
def cpu_cases():
    """[(name, dynamics, reward, value or None, w)]: case i uses activation i % 12 (code i % 12 + 1) in all three networks,
    mask i % 7 + 1, statistics on every other case, a value network on two cases of three."""
    out = []
    for i in range(14):
        a = ACT_NAMES[1 + i % 12]
        norm = i % 2 == 0
        last = ACT_NAMES[1 + (i + 5) % 12] if i % 3 == 0 else None      # a last-layer activation now and then ...
        if last not in ("tanh", "sigmoid", "elu", "softplus", "softsign", "swish"):
            last = None                                                  # ... of the kind that cannot switch the whole gradient off
        dyn = Dynamics("dyn-%s" % a, 3, 2, [20] if i % 2 else [20, 33], [a] * (1 if i % 2 else 2) + [last if last in ("tanh", "softsign") else None],
                       norm, 100 + i)
        rew = Stack("rew-%s" % a, 3, 2, i % 7 + 1, [33] if i % 2 else [20], [a, last], not norm if i % 4 == 1 else norm, 200 + i)
        val = Stack("val-%s" % a, 3, 2, 1, [20], [a, None], norm, 300 + i) if i % 3 != 2 else None
        out.append(("%02d-%s-mask%d-%s" % (i, a, i % 7 + 1, "norm" if norm else "raw"), dyn, rew, val, [1.0, -0.5, 0.0, 2.0][i % 4]))
    return out
