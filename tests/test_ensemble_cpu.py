"""Model ensembles with trajectory sampling, without a GPU: the NumPy statement the GPU tests compare against
(tests/ensemble_util.py) against tests/particle_util.py, the cases of the GPU test (built here once, so that the CPU check
of the cheetah margin rule and the GPU test see the same numbers), EnsembleMLP's save / load, ensemble training on the
host against DenseTrainer.fit called directly, residual_std, the constructor's refusal and the ABI's declaration."""
import ctypes
import functools
import os

import numpy as np
import pytest

from oracle import oracle_np as O
from tests import ensemble_util as EU
from tests import particle_util as PU

F = np.float32
SIGMA = 0.02                                    # process noise of the GPU cases (tests/test_gpu_particles.py's)
MARGIN_TOL = 2e-4                               # parity_util.assert_cheetah_rewards' default margin_tol
SWISH_NET = ([26, 200, 200, 20], ["swish", "swish", None], 20, 6, "cheetah")      # an activation after sigmoid: EXT kernels
# A narrow net with wide state and action: 16 hidden units run ONE wave of 64 threads, and the tiles [S][16] = 320 noise
# and [16][U] = 160 action elements exceed the 2 * 64 a workgroup holds in registers -- the only cases in which the particle
# kernels fetch noise and actions on their fall-back paths.  N 5, P 4: 20 rows per agent (a full and a partial tile), with
# E = 2 10 rows per member.  Checked on the CPU for every case built on it here, in tests/test_gaussian_cpu.py and in
# tests/test_gpu_particles.py (model seed 42, the input seeds those cases use): the float32 helper meets rtol / atol of the
# GPU tests against a float64 evaluation of the same recurrence on every row, and no visited state comes within margin_tol
# per step of an indicator threshold (smallest margin 5.6e-4), so assert_cheetah_rewards has no flip to let through.
NARROW_NET = ([30, 16, 16, 20], ["tanh", "tanh", None], 20, 10, "cheetah")
# (network, N, A, P, E, H, seed) of tests/test_gpu_ensemble.py::test_returns_match_the_helper
CASES = [("CHEETAH", 5, 1, 6, 3, 2, 42), ("CHEETAH", 37, 3, 4, 2, 12, 42), ("PEND_MLP", 33, 2, 16, 8, 9, 42),
         ("PEND_MLP", 33, 2, 3, 1, 9, 42), ("SWISH", 5, 1, 6, 3, 2, 42), ("NARROW", 5, 2, 4, 2, 3, 42)]


def network(name):
    from tests import test_gpu_mlp as TM
    return {"SWISH": SWISH_NET, "NARROW": NARROW_NET}.get(name) or getattr(TM, name)


def member_params(dims, seed, e):
    """Member e's parameters: tests/test_gpu_mlp._problem's recipe at seed + 10 e (member 0 is what _problem installs)."""
    ws, bs = O.make_mlp_params(dims, seed=seed + 10 * e)
    rng = np.random.default_rng(seed + 10 * e + 1)
    return ws, [rng.normal(0, 0.05, b.shape).astype(F) for b in bs]


def member_evaluators(spec, E, seed=42, normalized=True):
    """([(weights, biases)] per member, stats, [oracle Evaluator] per member): one shape, one set of statistics."""
    from tests.test_gpu_mlp import _stats
    dims, acts, S, U, reward = spec
    stats = _stats(S, U, seed + 2) if normalized else None
    params = [member_params(dims, seed, e) for e in range(E)]
    if all(a in ("tanh", "relu", "sigmoid", None) for a in acts):
        nets = [O.MLP(ws, bs, acts) for ws, bs in params]
    else:
        from tests.test_gpu_activations import MLP64
        nets = [MLP64(ws, bs, acts) for ws, bs in params]
    return params, stats, [O.Evaluator(reward, O.Handler(net, False, normalized, stats)) for net in nets]


@functools.lru_cache(maxsize=None)
def ensemble_case(case):
    """Everything test_returns_match_the_helper needs, computed once per process: the members, the inputs, and the
    helper's returns with the states it visited."""
    name, N, A, P, E, H, seed = CASES[case]
    spec = network(name)
    dims, acts, S, U, reward = spec
    params, stats, evs = member_evaluators(spec, E, seed)
    rng = np.random.default_rng(2000 + case)
    states = (O.cheetah_start_states(A, S) if reward == "cheetah" else O.pendulum_start_states(A)).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, U)).astype(F)
    eps = rng.standard_normal((A, P, H, S)).astype(F)
    sigma = np.full(S, SIGMA, F)
    want, visited = EU.ensemble_particle_returns(evs, states, seq, eps, sigma, P, keep_states=True)
    for arr in (states, seq, eps, sigma, want):
        arr.setflags(write=False)
    return dict(spec=spec, params=params, stats=stats, evs=evs, states=states, seq=seq, eps=eps, sigma=sigma, want=want,
                visited=visited, shape=(N, A, P, E, H))


def ensemble_margin(case):
    """particle_util.cheetah_noisy_margin on the helper's visited states, in the returns' layout [N, P, A]."""
    c = ensemble_case(case)
    N, A, P, E, H = c["shape"]
    out = np.empty((N, P, A))
    for e in range(E):
        out[:, e::E, :] = PU.cheetah_noisy_margin(c["visited"][e]).reshape(N, P // E, A)
    return out


# ---- the helper ------------------------------------------------------------------------------------------------------
def test_helper_with_copies_of_one_model_is_the_particle_helper():
    ws, bs = O.make_mlp_params([4, 16, 3], seed=1)
    ev = O.Evaluator("pendulum", O.Handler(O.MLP(ws, bs, ["tanh", None]), False, False))
    N, A, P, H = 9, 2, 6, 5
    rng = np.random.default_rng(0)
    states = O.pendulum_start_states(A)
    seq = rng.uniform(-2, 2, (N, A, H, 1)).astype(F)
    eps = rng.standard_normal((A, P, H, 3)).astype(F)
    sigma = np.array([0.01, 0.01, 0.05], F)
    want = PU.particle_returns(ev, states, seq, eps, sigma, P)
    for E in (1, 2, 3, 6):
        np.testing.assert_array_equal(EU.ensemble_particle_returns([ev] * E, states, seq, eps, sigma, P), want)
    pe = EU.EnsembleParticleEvaluator([ev] * 3, P, sigma, 1.5, eps)
    np.testing.assert_array_equal(pe(states, seq), PU.ParticleEvaluator(ev.reward, ev.handler, P, sigma, 1.5, eps)(states, seq))
    # ... and with two different models particle p carries member p % E: swapping the members swaps the particles
    ws2, bs2 = O.make_mlp_params([4, 16, 3], seed=2)
    ev2 = O.Evaluator("pendulum", O.Handler(O.MLP(ws2, bs2, ["tanh", None]), False, False))
    r12 = EU.ensemble_particle_returns([ev, ev2], states, seq, eps, sigma, P)
    np.testing.assert_array_equal(r12[:, 0::2], PU.particle_returns(ev, states, seq, eps[:, 0::2], sigma, P // 2))
    np.testing.assert_array_equal(r12[:, 1::2], PU.particle_returns(ev2, states, seq, eps[:, 1::2], sigma, P // 2))
    assert np.all(r12[:, 0] != r12[:, 1])


def _single_model_margin_fraction(N, A, P, H, seed):
    """What tests/test_gpu_particles.py::test_mlp_particle_returns_match_the_helper leaves to the margin rule on its own
    inputs (its cheetah case of that shape and seed, the model of test_gpu_mlp._problem): the fraction of rows whose
    noisy trajectory comes within margin_tol per step of an indicator threshold."""
    spec = network("CHEETAH")
    _, _, evs = member_evaluators(spec, 1)
    rng = np.random.default_rng(seed)
    states = O.cheetah_start_states(A, 20).astype(F)
    seq = rng.uniform(-1, 1, (N, A, H, 6)).astype(F)
    eps = rng.standard_normal((A, P, H, 20)).astype(F)
    _, visited = PU.particle_returns(evs[0], states, seq, eps, np.full(20, SIGMA, F), P, keep_states=True)
    return float((PU.cheetah_noisy_margin(visited) <= MARGIN_TOL).mean())


# ensemble case -> the single-model test's case of the same N, A, H: (N, A, P, H, seed)
_SINGLE_MODEL_CASE = {0: (5, 1, 3, 2, 1000), 1: (37, 3, 4, 12, 1001), 4: (5, 1, 3, 2, 1000)}


@pytest.mark.parametrize("case", sorted(_SINGLE_MODEL_CASE))
def test_gpu_cases_leave_no_more_rows_to_the_margin_rule_than_the_single_model_test(case):
    """The GPU test lets a cheetah return miss the tolerance only by indicator flips, and only on rows whose (noisy)
    trajectory comes within margin_tol per step of a threshold.  The cheetah start states sit near two of the three
    thresholds, so such rows exist in every case; the cap on their share is what the single-model particle test leaves on
    its own inputs at the same shape (a quarter of the rows at H = 12, none at H = 2).  Every other row has to meet
    rtol / atol on the device -- a wrong row -> member or row -> store map moves at least a whole member's rows."""
    c = ensemble_case(case)
    assert np.all(np.isfinite(c["want"]))
    margin = ensemble_margin(case)
    share, cap = float((margin <= MARGIN_TOL).mean()), _single_model_margin_fraction(*_SINGLE_MODEL_CASE[case])
    print("[ensemble case %d] smallest margin %.3e, rows within margin_tol: %.3f (single-model test: %.3f)"
          % (case, margin.min(), share, cap))
    assert share <= cap
    # the members disagree: the returns of one candidate differ between particles of different members
    assert np.all(c["want"][:, 0] != c["want"][:, 1])


# ---- EnsembleMLP -----------------------------------------------------------------------------------------------------
def test_ensemble_mlp_is_member_0_to_deterministic_consumers_and_round_trips(tmp_path):
    from blackbox_mpc_amd.dynamics_functions import DeterministicMLP, EnsembleMLP
    ens = EnsembleMLP([4, 16, 16, 3], ["tanh", "swish", None], num_members=3, seed=5)
    assert ens.num_members == 3 and len(ens.members) == 3 and all(isinstance(m, DeterministicMLP) for m in ens.members)
    assert ens.weights is ens.members[0].weights and ens.biases is ens.members[0].biases
    assert ens.activation_codes == ens.members[0].activation_codes and ens.layer_sizes == [4, 16, 16, 3]
    for i in range(3):
        for j in range(i + 1, 3):
            assert not np.array_equal(ens.members[i].weights[0], ens.members[j].weights[0])
    again = EnsembleMLP([4, 16, 16, 3], ["tanh", "swish", None], num_members=3, seed=5)
    for m, n in zip(ens.members, again.members):
        np.testing.assert_array_equal(m.weights[1], n.weights[1])
    v = ens._version
    ens.members[2].set_weights(ens.members[2].weights, [b + F(1) for b in ens.members[2].biases])
    assert ens._version == v + 1                          # any member's refit is a new version
    for bad in (0, 9):
        with pytest.raises(ValueError):
            EnsembleMLP([4, 8, 3], ["tanh", None], num_members=bad)
    d = str(tmp_path / "model")
    ens.save(d)
    assert sorted(os.listdir(d)) == ["mlp.npz", "mlp_member1.npz", "mlp_member2.npz"]
    back = EnsembleMLP.load(d)
    assert back.num_members == 3 and back.activation_codes == ens.activation_codes
    for m, n in zip(ens.members, back.members):
        for x, y in zip(m.weights + m.biases, n.weights + n.biases):
            np.testing.assert_array_equal(x, y)
    plain = DeterministicMLP.load(os.path.join(d, "mlp.npz"))            # the directory also loads as a plain model
    for x, y in zip(plain.weights + plain.biases, ens.members[0].weights + ens.members[0].biases):
        np.testing.assert_array_equal(x, y)
    EnsembleMLP.from_members(ens.members[:2]).save(d)                     # a smaller ensemble over a larger one
    assert EnsembleMLP.load(d).num_members == 2


def _ensemble_handler(E=3, normalized=True, seed=3, **kw):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions import EnsembleMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    fn = EnsembleMLP([4, 16, 16, 3], ["tanh", "relu", None], num_members=E, seed=seed)
    h = SystemDynamicsHandler(Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]), dynamics_function=fn,
                              is_normalized=normalized, **kw)
    return h, fn


def test_handler_save_and_load_round_trip_the_ensemble(tmp_path):
    from blackbox_mpc_amd import Box
    from blackbox_mpc_amd.dynamics_functions import DeterministicMLP, EnsembleMLP
    from blackbox_mpc_amd.dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
    h, fn = _ensemble_handler(E=2)
    h.set_normalization_stats(*[np.full(n, 0.5 + i, F) for i, n in enumerate((3, 3, 1, 1, 3, 3))])
    h.save(str(tmp_path))
    spaces = (Box(low=[-2.0], high=[2.0]), Box(low=[-1, -1, -8], high=[1, 1, 8]))
    back = SystemDynamicsHandler(*spaces, saved_model_dir=str(tmp_path))
    assert isinstance(back._dynamics_function, EnsembleMLP) and back._dynamics_function.num_members == 2
    for m, n in zip(fn.members, back._dynamics_function.members):
        for x, y in zip(m.weights + m.biases, n.weights + n.biases):
            np.testing.assert_array_equal(x, y)
    for x, y in zip(h.normalization_stats(), back.normalization_stats()):
        np.testing.assert_array_equal(x, y)
    os.remove(str(tmp_path / "mlp_member1.npz"))
    assert isinstance(SystemDynamicsHandler(*spaces, saved_model_dir=str(tmp_path))._dynamics_function, DeterministicMLP)


@pytest.mark.parametrize("normalized", [True, False])
def test_ensemble_training_is_dense_trainer_fit_on_the_bootstrap_rows(normalized):
    from blackbox_mpc_amd.dynamics_functions._train_torch import DenseTrainer
    from tests.test_train_cpu import _episodes
    obs, acs, rews = _episodes(4, 40, 2, 2)
    E, epochs, batch, lr = 3, 3, 32, 2e-3
    h, fn = _ensemble_handler(E, normalized)
    start = [([w.copy() for w in m.weights], [b.copy() for b in m.biases]) for m in fn.members]
    rng = np.random.default_rng(4)
    mask = rng.random(4 * 2 * 40) > 0.25
    n = int(mask.sum())
    boot = rng.integers(0, n, size=(E, n))
    perms = [[rng.permutation(n) for _ in range(epochs)] for _ in range(E)]
    h.train(obs, acs, rews, batch_size=batch, learning_rate=lr, epochs=epochs, device="cpu", seed=7, split_mask=mask,
            permutations=perms, bootstrap_indices=boot)
    tin, tout = h._normalize_data(h._model_training_in, h._model_training_out)
    vin, vout = h._normalize_data(h._model_validation_in, h._model_validation_out)
    assert tin.shape[0] == n
    rms = []
    for e in range(E):
        tr = DenseTrainer(start[e][0], start[e][1], fn.activation_codes, "cpu", learning_rate=lr, rule="adam")
        tl, vl = tr.fit(tin[boot[e]], tout[boot[e]], vin, vout, epochs, batch, permutations=perms[e], generator_seed=7)
        ws, bs = tr.numpy_params()
        for x, y in zip(ws + bs, fn.members[e].weights + fn.members[e].biases):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(h.member_training_loss[e], tl)
        np.testing.assert_array_equal(h.member_validation_loss[e], vl)
        assert not np.array_equal(ws[0], start[e][0][0])                 # it trained
        rms.append(tr.residual_rms(vin, vout).astype(np.float64))
    np.testing.assert_array_equal(h.training_loss, h.member_training_loss[0])
    np.testing.assert_array_equal(h.validation_loss, h.member_validation_loss[0])
    for i in range(E):
        for j in range(i + 1, E):
            assert not np.array_equal(fn.members[i].weights[-1], fn.members[j].weights[-1])
    # residual_std: the RMS over members of the members' validation residuals, in state units
    want = np.sqrt(np.mean(np.square(np.array(rms)), axis=0))
    if normalized:
        want = want * (h.normalization_stats()[5].astype(np.float64) + 1e-7)
    got = h.residual_std()
    assert got.shape == (3,) and got.dtype == np.float32
    np.testing.assert_allclose(got, want, rtol=1e-6)


def test_ensemble_training_draws_its_own_bootstrap_from_the_seed():
    from tests.test_train_cpu import _episodes
    obs, acs, rews = _episodes(2, 40, 2, 2)
    mask = np.random.default_rng(1).random(2 * 2 * 40) > 0.25
    runs = []
    for seed in (11, 11, 12):
        h, fn = _ensemble_handler(E=2)
        h.train(obs, acs, rews, batch_size=32, epochs=2, device="cpu", seed=seed, split_mask=mask)
        runs.append([m.weights[0].copy() for m in fn.members])
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert not np.array_equal(runs[0][0], runs[2][0])
    # the plain model's path refuses the ensemble's keyword
    from tests.test_train_cpu import _handler
    with pytest.raises(ValueError, match="bootstrap_indices"):
        _handler()[0].train(obs, acs, rews, epochs=1, device="cpu", bootstrap_indices=[[0]])
    with pytest.raises(ValueError, match="bootstrap_indices"):
        _ensemble_handler(E=2)[0].train(obs, acs, rews, epochs=1, device="cpu", split_mask=mask, bootstrap_indices=[[0]])


def test_particle_evaluator_refuses_particles_that_do_not_divide():
    from blackbox_mpc_amd.trajectory_evaluators import ParticleTrajectoryEvaluator
    from blackbox_mpc_amd.utils.pendulum import pendulum_reward_function
    h, fn = _ensemble_handler(E=3)
    with pytest.raises(ValueError, match="num_members"):
        ParticleTrajectoryEvaluator(pendulum_reward_function, h, num_particles=4, process_noise_std=0.1)
    ev = ParticleTrajectoryEvaluator(pendulum_reward_function, h, num_particles=6, process_noise_std=0.1, risk_kappa=1.0)
    assert ev.particle_settings[0] == 6


def test_header_declares_and_the_binding_names_the_setter():
    from blackbox_mpc_amd import _build
    _build.build()
    from blackbox_mpc_amd import _lib as L
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bbmpc.h")).read()
    assert "int bbmpc_set_mlp_ensemble(" in header and "bbmpc_set_mlp_ensemble" in L.SYMBOLS
    assert hasattr(L.lib, "bbmpc_set_mlp_ensemble") and L.MAX_ENSEMBLE_MEMBERS == 8
    assert L.lib.bbmpc_set_mlp_ensemble(None, 2, None, None) == L.E_INVALID and b"null handle" in L.lib.bbmpc_last_error()
    from blackbox_mpc_amd.engine import Engine
    assert callable(Engine.set_mlp_ensemble)
