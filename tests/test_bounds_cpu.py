"""CPU checks of the inputs of tests/test_gpu_optimizer_bounds.py, on the oracle alone: under every bound set and for every
optimizer of those tests the free-running oracle, fed the very draws and start states the GPU cases use, must exercise what
the GPU tests claim to compare -- candidates clipped on both sides with a non-zero penalty, a bound-constrained variance
below the unconstrained one on either side of the midpoint, uniform draws at both ends of [0, 1) -- so that no GPU case can
pass vacuously.  Also pins tests/bounds_util.py itself (check_candidates, the coverage counts)."""
import numpy as np
import pytest

from tests import bounds_util as B

F = np.float32


def case(name):
    """(evaluator, lo, hi, states [STEPS, A, S]) -- bounds_util.problem, which the GPU tests build their cases from too"""
    return B.problem(name)[:4]


_RUNS = {}


def run(name, opt_name):
    """computed once per (case, optimizer), shared by the tests below, never changed"""
    if (name, opt_name) not in _RUNS:
        ev, lo, hi, states = case(name)
        _RUNS[name, opt_name] = B.run_oracle(opt_name, ev, lo, hi, states, B.case_seed(name, opt_name), mix=B.case_mix(name))
    return _RUNS[name, opt_name]


SETS = list(B.PENDULUM_SETS) + list(B.LEARNED_CASES)
KSETS = SETS + list(B.KERNEL_CASES)                       # ... and the problems of the RS / CEM / PI2 cases of the other kernels


def _all_clips(r):
    return [c for step in r.clips for c in step]


@pytest.mark.parametrize("name", KSETS)
def test_pi2_clips_on_both_sides_in_every_dimension_with_a_penalty(name):
    r, _ = run(name, "PI2")
    cov = B.clip_coverage(_all_clips(r), r.lo, r.hi)
    print("[bounds coverage] PI2 %s: at_hi %s at_lo %s penalised rows %s" % (name, cov["at_hi"], cov["at_lo"], cov["penalised"]))
    assert np.all(cov["at_hi"] >= 1) and np.all(cov["at_lo"] >= 1), cov
    assert np.all(cov["penalised"] >= 1), cov
    assert max(float(t["penalty"].max()) for t in r.opt.trace) > 0.0          # (the last control step's trace)


def _update_never_clips(cu):
    # the claim "some solution element is clipped by the a_k * ghat update" is dropped for EVERY set: a_k <= 0.0085 times
    # the gradient estimates these rewards give never carries the solution over a bound within the case's iterations, so
    # the GPU cases compare the update on unclipped solutions only.  Asserted, so that a change of inputs that makes the
    # update clip is noticed and the claim can be reinstated
    assert (cu["at_hi"] + cu["at_lo"]).sum() == 0, cu


@pytest.mark.parametrize("name", SETS)
def test_spsa_clips_both_candidates_where_the_range_is_below_its_reach(name):
    r, _ = run(name, "SPSA")
    narrow = (r.hi.astype(np.float64) - r.lo.astype(np.float64)) < B.SPSA_REACH
    per_it = [c for step in r.clips for c in step]
    plus, minus, upd = per_it[0::3], per_it[1::3], per_it[2::3]
    cp, cm, cu = (B.clip_coverage(x, r.lo, r.hi) for x in (plus, minus, upd))
    print("[bounds coverage] SPSA %s: narrow dims %s plus hi/lo %s/%s minus hi/lo %s/%s update hi/lo %s/%s" % (
        name, np.flatnonzero(narrow), cp["at_hi"], cp["at_lo"], cm["at_hi"], cm["at_lo"], cu["at_hi"], cu["at_lo"]))
    if name in B.SPSA_OUT_OF_REACH:
        _update_never_clips(cu)
        # every dimension is at least 2 c_0 wide and the solution stays away from the bounds over the case's iterations:
        # nothing clips, and the GPU test of this set claims no clip coverage for SPSA (the issue's own finding)
        assert not narrow.any()
        return
    assert narrow.any(), "the set must have a dimension narrower than 2 c_0"
    for c in (cp, cm):
        assert np.all((c["at_hi"] + c["at_lo"])[narrow] >= 1), c          # both perturbed candidates leave the bounds there
        assert np.all(c["penalised"][narrow] >= 1), c
    # the two candidates leave on opposite sides: together both bounds are hit in every narrow dimension
    assert np.all((cp["at_hi"] + cm["at_hi"])[narrow] >= 1) and np.all((cp["at_lo"] + cm["at_lo"])[narrow] >= 1)
    _update_never_clips(cu)


VAR_CASES = [(n, o) for n in SETS for o in ("CEM", "CEM-warm", "PSO", "PSO-reset")] + \
            [(n, "CEM") for n in B.KERNEL_CASES if B.case_mix(n) is None]      # (correlated CEM clips its mixed draws instead: PI2's test)


@pytest.mark.parametrize("name,opt_name", VAR_CASES)
def test_constrained_variance_binds_on_both_sides_of_the_midpoint(name, opt_name):
    r, var_cov = run(name, opt_name)
    near_lo, near_hi = sum(v["near_lo"] for v in var_cov), sum(v["near_hi"] for v in var_cov)
    print("[bounds coverage] %s %s: constrained variance below the unconstrained one at %d elements nearer lo, %d nearer hi" % (
        opt_name, name, near_lo, near_hi))
    if opt_name == "PSO" and name not in B.PSO_Q4_BOTH_SIDES:
        # quirk Q4 (no reset()): pbest = 0 with pbest_r = 0 comes from the constructor and no (negative) reward beats it, so
        # gbest stays the all-zero pbest -- below the midpoint in every dimension of these sets (0 < midpoint[u]) -- and the
        # re-seed is drawn around it.  The upper arm is out of reach there; PSO-reset covers it
        assert near_lo >= 1 and near_hi == 0, (near_lo, near_hi)
        return
    assert near_lo >= 1 and near_hi >= 1, (near_lo, near_hi)


@pytest.mark.parametrize("U", [1, 2, 6, 64])
def test_injected_uniforms_hold_both_ends_in_every_dimension(U):
    for opt_name in ("RS", "PSO-reset"):
        reset, draws = B.case_draws(opt_name, B.A, U, 3)
        tensors = [d["uniform"] for d in draws] + ([reset["uniform_pos"], reset["uniform_vel"]] if reset else [])
        for u01 in tensors:
            assert u01.dtype == F and u01.min() >= 0 and u01.max() < 1
            flat = u01.reshape(-1, U)
            assert np.all((flat == 0).any(0)) and np.all((flat == B.ONE_BELOW).any(0))
    assert B.ONE_BELOW == F(1) - F(2.0 ** -24) and B.ONE_BELOW < 1


@pytest.mark.parametrize("name", KSETS)
def test_uniform_map_reaches_both_bounds_and_stays_inside(name):
    ev, lo, hi, states = case(name)
    r, _ = run(name, "RS")
    s = r.opt.trace[0]["samples"]
    B.check_candidates(s, s, lo, hi, 1e-5)
    flat = s.reshape(-1, lo.shape[0])
    assert np.all((flat == lo).any(0))                   # u = 0 gives lo[u] exactly
    assert np.all((flat >= hi - F(1e-6)).any(0))         # u = 1 - 2^-24 gives hi[u] to rounding, never more
    if name in B.KERNEL_CASES:
        return
    r, _ = run(name, "PSO-reset")                        # the reset map (pso.py:143-160) read back after the first clip
    first = r.clips[0][0]
    B.check_candidates(first, first, lo, hi, 1e-5)


@pytest.mark.parametrize("opt_name", ["CMA", "CMA-pa"])
@pytest.mark.parametrize("name", SETS)
def test_cmaes_candidates_are_clipped_in_every_dimension(name, opt_name):
    r, _ = run(name, opt_name)
    cov = B.clip_coverage(_all_clips(r), r.lo, r.hi)
    print("[bounds coverage] %s %s: at_hi %s at_lo %s" % (opt_name, name, cov["at_hi"], cov["at_lo"]))
    assert np.all(cov["at_hi"] >= 1) and np.all(cov["at_lo"] >= 1), cov          # N(0,1) draws at sigma = range / 4


def test_check_candidates_catches_what_it_is_for():
    lo, hi = B.mlp_bounds(2)
    raw = np.array([[[1.6, 0.5], [-0.7, 0.2]], [[0.3, 0.9], [1.0, 0.3]]], F)          # [2, 2, U]
    want = np.clip(raw, lo, hi)
    got = want.copy()
    at_hi, at_lo, inside = B.check_candidates(got, want, lo, hi, 1e-5, raw=raw)
    assert at_hi.tolist() == [1, 1] and at_lo.tolist() == [1, 1] and inside.tolist() == [2, 2]
    for idx, val in (((0, 0, 0), 1.5 - 1e-6),          # a clipped element that is merely close to hi
                     ((0, 1, 0), 0.25),                # lo of the OTHER dimension
                     ((1, 0, 0), 0.3 + 3e-5),          # off by more than atol
                     ((1, 1, 1), 0.25 - 1e-6)):        # inside atol of the oracle but outside the bounds
        bad = want.copy()
        bad[idx] = val
        with pytest.raises(AssertionError):
            B.check_candidates(bad, want if idx != (1, 1, 1) else bad, lo, hi, 1e-5, raw=raw)
    # the coverage counts, on the same tensor read as [rows, H, U]: row 0 leaves the bounds in both dimensions (twice in
    # u = 0: still one penalised row), row 1 in u = 1 only
    cov = B.clip_coverage([raw], lo, hi)
    assert cov["at_hi"].tolist() == [1, 1] and cov["at_lo"].tolist() == [1, 1] and cov["penalised"].tolist() == [1, 2]
    cv, lo_side, hi_side = B.constrained_variance(np.array([[[0.0, 0.7]]], F), np.array([[[0.25, 0.25]]], F), lo, hi)
    np.testing.assert_allclose(cv, [[[0.0625, 0.000625]]], rtol=1e-6)
    assert lo_side.tolist() == [[[True, False]]] and hi_side.tolist() == [[[False, True]]]
