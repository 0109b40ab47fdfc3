"""NaN candidates among ordinary ones: the poison patterns and the one assertion every scorer of candidates is held to.

The reference evaluator ends with one rule (deterministic.py:75-77): a trajectory whose reward sum is NaN scores exactly
-1e6.  Every candidate is a separate row of its batch, so the NaN has no other effect.  On the device several candidates
share a wave, zero-padded lanes take part in matrix products and values move between lanes; a wrong mask or rotation is
invisible on finite data where its contribution is 0 * x, and turns a neighbour into NaN once x is NaN.

patterns(seq) returns poisoned copies of action sequences [N, A, H, U] with, for each, the set of poisoned (n, a);
check(clean, poisoned, set) states the contract bit for bit: -1e6 exactly inside the set, the clean run's bits outside it.
NaN goes into action values only -- never into anything a kernel uses as an index or a count."""
import numpy as np

F = np.float32
MINUS_1E6 = F(-1e6)


def patterns(seq):
    """seq [N, A, H, U] -> list of (name, poisoned copy, set of poisoned (n, a)), each for one evaluate call.
    first : seq[0, 0, 0, 0]
    last  : seq[N-1, A-1, H-1, U-1] -- the ragged last particle, the last step, the last action slot
    comb  : every n with n % 4 == 1, agent 0, step H // 2, the action slot alternating between 0 and U-1: one poisoned
            particle in every quad and several in every 16-tile, each with clean neighbours on both sides
    agent : (A >= 2 and N > 17) n = 17, agent 1 only"""
    seq = np.asarray(seq, F)
    N, A, H, U = seq.shape
    out = []
    p = seq.copy()
    p[0, 0, 0, 0] = np.nan
    out.append(("first", p, {(0, 0)}))
    p = seq.copy()
    p[N - 1, A - 1, H - 1, U - 1] = np.nan
    out.append(("last", p, {(N - 1, A - 1)}))
    p, hit = seq.copy(), set()
    for i, n in enumerate(range(1, N, 4)):
        p[n, 0, H // 2, (U - 1) if i % 2 else 0] = np.nan
        hit.add((n, 0))
    if hit:
        out.append(("comb", p, hit))
    if A >= 2 and N > 17:
        p = seq.copy()
        p[17, 1, :, :] = np.nan
        out.append(("agent", p, {(17, 1)}))
    for _, p, hit in out:                       # the sets name exactly the candidates that hold a NaN
        bad = np.isnan(p).any(axis=(2, 3))
        assert {(int(n), int(a)) for n, a in zip(*np.nonzero(bad))} == hit
    return out


GPU_N, GPU_A = 37, 2       # the rollout shape of tests/test_gpu_nonfinite_candidates.py: two full 16-tiles plus 5, nine quads plus 1

# (id, dims, activations) of the one-step cases: the cheetah network, the pendulum network, one activation after sigmoid
STEP_NETS = [("cheetah", [26, 200, 200, 20], ["tanh", "tanh", None]),
             ("pendulum", [4, 32, 32, 32, 3], ["tanh", "tanh", "tanh", None]),
             ("cheetah_ext", [26, 200, 200, 20], ["elu", "tanh", None])]


def gpu_shape(c):
    """a rollout case of tests/test_gpu_mlp_kernel_choice.py at N = 37, A = 2, with the case's own horizon"""
    return dict(c, N=GPU_N, A=GPU_A)


def step_inputs(c, B):
    """-> (states [B, S], actions [B, U]) of a one-step case (pendulum states on the unit circle)"""
    rng = np.random.default_rng(sum(c["dims"]) + B)
    s = rng.normal(0, 0.5, (B, c["S"])).astype(F)
    if c["reward"] == "pendulum":
        th = rng.uniform(-np.pi, np.pi, B)
        s = np.stack([np.cos(th), np.sin(th), rng.uniform(-4, 4, B)], 1).astype(F)
    return s, rng.uniform(-1, 1, (B, c["U"])).astype(F)


def bounded_normal_draws(rng, shape, limit=0.8):
    """Normal draws resampled until |z| < 2, times limit / 2: CMA-ES candidates m + sigma (z B D) that stay inside the action
    bounds for the first iterations from the constructor's state (m the midpoint, sigma a quarter of the range, B D = I),
    so that no bound penalty is subtracted from a score."""
    z = rng.standard_normal(shape)
    bad = np.abs(z) >= 2.0
    while bad.any():
        z[bad] = rng.standard_normal(int(bad.sum()))
        bad = np.abs(z) >= 2.0
    return (z * (limit / 2.0)).astype(F)


def mask_of(shape, poisoned):
    m = np.zeros(shape, bool)
    for n, a in poisoned:
        m[n, a] = True
    return m


def check(got_clean, got_poisoned, poisoned, what=""):
    """Rewards [N, A] of one engine without and with the poison: entries in the set are float32(-1e6) exactly, all others
    are the clean run's bits.  No tolerance and no allowed share of exceptions."""
    clean, got = np.asarray(got_clean), np.asarray(got_poisoned)
    assert clean.dtype == F and got.dtype == F and clean.shape == got.shape and clean.ndim == 2, (clean.dtype, got.dtype, clean.shape, got.shape)
    assert len(poisoned) > 0
    assert not np.isnan(clean).any(), "%s: the clean run holds NaN" % what
    assert not (clean == MINUS_1E6).any(), "%s: a clean reward is -1e6 itself" % what
    m = mask_of(clean.shape, poisoned)
    wrong = np.nonzero(m & ~(got == MINUS_1E6))
    assert wrong[0].size == 0, "%s: poisoned candidates that do not score -1e6: %s -> %s" % (
        what, list(zip(*[w.tolist() for w in wrong]))[:8], got[wrong][:8])
    np.testing.assert_array_equal(np.where(m, F(0), got), np.where(m, F(0), clean),
                                  err_msg="%s: a NaN candidate changed another candidate's reward" % what)
    # (assert_array_equal takes +0 == -0; the bits say the rest)
    np.testing.assert_array_equal(got.view(np.uint32)[~m], clean.view(np.uint32)[~m],
                                  err_msg="%s: a NaN candidate changed another candidate's bits" % what)


def check_rows(clean, poisoned_out, want_rows, rows, what=""):
    """The one-step forms on rows [B, ...]: the poisoned rows equal `want_rows` (the oracle's, NaN equal to NaN), every
    other row is the clean call's bits."""
    clean, got = np.asarray(clean), np.asarray(poisoned_out)
    assert clean.dtype == F and got.dtype == F and clean.shape == got.shape
    assert not np.isnan(clean).any(), "%s: the clean call holds NaN" % what
    rows = sorted(rows)
    np.testing.assert_array_equal(got[rows], np.asarray(want_rows, F), err_msg="%s: poisoned rows" % what)
    keep = np.ones(clean.shape[0], bool)
    keep[rows] = False
    np.testing.assert_array_equal(got[keep].view(np.uint32), clean[keep].view(np.uint32),
                                  err_msg="%s: a NaN row changed another row's bits" % what)
