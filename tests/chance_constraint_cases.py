"""The random-network cases of the chance constraint's tests, computed once per process and shared by the CPU test (which
checks the precondition on the bound) and the GPU test (which runs them): PEND_MLP (3 + 1 -> 3, tanh) as one model, as an
ensemble of two and with log-variance heads, under the built-in pendulum reward and under a HIP-source reward."""
import functools

import numpy as np

from oracle import oracle_np as O
from tests import chance_constraint_util as CC
from tests import ensemble_util as EU
from tests import gaussian_util as GU
from tests import particle_user_reward_util as RU
from tests import particle_util as PU
from tests.traj_util import STATE_ATOL, STATE_RTOL

F = np.float32
N, A, P, H = 13, 2, 4, 5
SIGMA = np.full(3, 0.02, F)
DELTA, WEIGHT = 0.25, 7.5
FEATURE, QUANTILE = 2, 0.75
# (kind, reward, input seed): seeds for which the precondition below holds (tests/test_chance_constraint_cpu.py checks it)
CASES = [("plain", "builtin", 5115), ("plain", "user", 5101), ("ens", "builtin", 5102), ("ens", "user", 5103),
         ("gauss", "builtin", 5104), ("gauss", "user", 5105), ("ensgauss", "builtin", 5106)]


@functools.lru_cache(maxsize=None)
def case(index):
    """-> dict: members' parameters, statistics, heads, inputs, the statement's returns [N,P,A], trajectories [H,N,P,A,S],
    the chosen box, its half gap, first [N,P,A] and v [N,A]."""
    from tests.test_ensemble_cpu import member_evaluators, network
    from tests.test_gaussian_cpu import member_heads
    kind, reward, seed = CASES[index]
    E = 2 if kind in ("ens", "ensgauss") else 1
    heads = kind in ("gauss", "ensgauss")
    spec = network("PEND_MLP")
    params, stats, evs = member_evaluators(spec, E)
    if reward == "user":
        evs = [O.Evaluator(RU.mixed_np, ev.handler) for ev in evs]
    rng = np.random.default_rng(seed)
    states = O.pendulum_start_states(A).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, 1)).astype(F)
    eps = rng.standard_normal((A, P, H, 3)).astype(F)
    raw = bounds = None
    if heads:
        raw, bounds, hs = member_heads(spec, evs)
        returns, visited = GU.gaussian_particle_returns(evs, hs, states, seq, eps, SIGMA, P, keep_states=True)
        traj = CC.member_trajectories(visited, N, P, A)
    elif E > 1:
        returns, visited = EU.ensemble_particle_returns(evs, states, seq, eps, SIGMA, P, keep_states=True)
        traj = CC.member_trajectories(visited, N, P, A)
    else:
        returns, visited = PU.particle_returns(evs[0], states, seq, eps, SIGMA, P, keep_states=True)
        traj = CC.trajectories(visited, N, P, A)
    bound, half_gap = CC.pick_upper_bound(traj, FEATURE, QUANTILE)
    lo = np.full(3, -np.inf, F)
    hi = np.full(3, np.inf, F)
    hi[FEATURE] = F(bound)
    first = CC.first_steps(traj, lo, hi)
    out = dict(kind=kind, reward=reward, E=E, heads=heads, spec=spec, params=params, stats=stats, raw_heads=raw, head_bounds=bounds,
               states=states, seq=seq, eps=eps, returns=returns, traj=traj, lo=lo, hi=hi, bound=float(hi[FEATURE]),
               half_gap=float(half_gap) - abs(float(hi[FEATURE]) - bound), first=first, v=CC.violation(first))
    for arr in (states, seq, eps, returns, traj, first, out["v"]):
        arr.setflags(write=False)
    return out


def state_tolerance(bound):
    """What the suites allow between a device state and the NumPy statement's (tests/traj_util.py)."""
    return STATE_ATOL + STATE_RTOL * abs(bound)
