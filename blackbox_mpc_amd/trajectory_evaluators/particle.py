"""ParticleTrajectoryEvaluator -- the "different trajectory evaluators to propagate uncertainties" the reference's
README leaves open (its EvaluatorBase / set_trajectory_evaluator layout was made for them): every candidate is rolled out
`num_particles` times through the ONE model with additive Gaussian process noise on the predicted next state, and the
returns are reduced to  mean - risk_kappa * std  (include/bbmpc.h: bbmpc_set_particles).  The noise does not depend on
the candidate (common random numbers), so candidates of an agent are ranked on the same noise paths.  When the handler's
dynamics function is an EnsembleMLP, particle p follows member p % num_members for the whole horizon (trajectory
sampling, bbmpc_set_mlp_ensemble): the spread of the returns then carries the members' disagreement as well.  When it is
a ProbabilisticMLP, or an ensemble of them, the noise scale of a step is process_noise_std plus the standard deviation
the model's log-variance head predicts at that state and action (bbmpc_set_mlp_logvar_head), and process_noise_std = 0
-- the learned noise alone -- is a sensible setting.

risk_alpha in (0, 1] replaces mean - risk_kappa * std by the conditional value at risk of the lower tail: the mean of the
k = ceil(risk_alpha * num_particles) worst returns (bbmpc_set_particle_risk), which tells a candidate that crashes in a
few particles from one that wobbles in all of them and does not punish upside spread.  predict_trajectory_distribution
(..., quantiles=[0.05, 0.95]) adds nearest-rank quantile bands to the mean / std ones."""
import math

import numpy as np

from .. import _lib as L

from .deterministic import DeterministicTrajectoryEvaluator


def cvar_tail_count(alpha, num_particles):
    """k = min(P, max(1, ceil(alpha P - 1e-9))) for alpha in (0, 1]: the number of worst returns CVaR_alpha averages.
    Python floats; the engine sees only the integer (the 1e-9 keeps 0.1 * 10 = 1.0000000000000002 at 1)."""
    a = float(alpha)
    if not (math.isfinite(a) and 0.0 < a <= 1.0):
        raise ValueError("risk_alpha must lie in (0, 1], got %r" % (alpha,))
    p = int(num_particles)
    return min(p, max(1, math.ceil(a * p - 1e-9)))


def quantile_rank(tau, num_particles):
    """Nearest rank of level tau in (0, 1] among P values: min(P - 1, max(0, ceil(tau P - 1e-9) - 1))."""
    t = float(tau)
    if not (math.isfinite(t) and 0.0 < t <= 1.0):
        raise ValueError("a quantile level must lie in (0, 1], got %r" % (tau,))
    p = int(num_particles)
    return min(p - 1, max(0, math.ceil(t * p - 1e-9) - 1))


def _constraint_version(evaluator):
    c = getattr(evaluator, "_constraint", None)
    return (id(c), getattr(c, "_version", 0))


def configure_constraint(engine, evaluator):
    """Upload the evaluator's StateBoxConstraint (constraint=) behind set_particles; nothing to do without one."""
    c = getattr(evaluator, "_constraint", None)
    if c is None:
        return
    lo, hi = c.bounds(engine.S)
    engine.set_chance_constraint(lo, hi, c.max_violation, c.weight)
    engine._constraint_version = _constraint_version(evaluator)


def constraint_stale(engine, evaluator):
    """A box whose bounds, limit or weight changed since they were uploaded (or that was never uploaded to this engine)."""
    return getattr(evaluator, "_constraint", None) is not None and engine.__dict__.get("_constraint_version") != _constraint_version(evaluator)


class ParticleTrajectoryEvaluator(DeterministicTrajectoryEvaluator):
    def __init__(self, reward_function, system_dynamics_handler, num_particles, process_noise_std, risk_kappa=0.0,
                 quirks=0, risk_alpha=None, terminal_value=None, terminal_weight=1.0, discount=1.0, termination=None,
                 constraint=None):
        """process_noise_std: a scalar or [dim_S], >= 0 -- for a learned model SystemDynamicsHandler.residual_std() is
        the natural choice.  risk_kappa > 0 prefers candidates whose return varies little over the particles.
        risk_alpha in (0, 1] scores the mean of the ceil(risk_alpha * num_particles) worst returns instead (CVaR; not
        together with risk_kappa != 0).  constraint: a utils.constraints.StateBoxConstraint -- a candidate's score then
        loses weight * max(0, v - max_violation), v the share of its particles whose noisy state ever leaves the box
        (learned dynamics with a built-in or HIP-source reward; bbmpc_set_chance_constraint)."""
        if getattr(reward_function, "_bbmpc_reward_kind", None) == L.REW_MLP:
            raise NotImplementedError("ParticleTrajectoryEvaluator does not score a LearnedRewardMLP yet: the particle rollouts take "
                                      "built-in and HIP-source rewards (use DeterministicTrajectoryEvaluator with a learned reward)")
        if terminal_value is not None:
            raise NotImplementedError("ParticleTrajectoryEvaluator has no terminal term yet: a LearnedValueMLP closes the rollouts of "
                                      "DeterministicTrajectoryEvaluator only")
        if termination is not None or float(discount) != 1.0:
            raise NotImplementedError("ParticleTrajectoryEvaluator has no discounted or termination-aware return yet: discount / "
                                      "termination shape the rollouts of DeterministicTrajectoryEvaluator only")
        super().__init__(reward_function, system_dynamics_handler, quirks=quirks)
        p = int(num_particles)
        if not 1 <= p <= 64:
            raise ValueError("num_particles must be in [1, 64], got %r" % (num_particles,))
        dim_s = system_dynamics_handler._dim_S
        sg = np.asarray(process_noise_std, np.float32)
        sg = np.full((dim_s,), sg, np.float32) if sg.ndim == 0 else sg.reshape(-1).astype(np.float32)
        if sg.shape != (dim_s,) or not np.all(np.isfinite(sg)) or np.any(sg < 0):
            raise ValueError("process_noise_std must be a finite scalar or [dim_S] = [%d] vector >= 0" % dim_s)
        if not np.isfinite(risk_kappa):
            raise ValueError("risk_kappa must be finite")
        members = getattr(system_dynamics_handler._dynamics_function, "members", None)
        if members is not None and p % len(members) != 0:
            raise ValueError("num_particles = %d is no multiple of the EnsembleMLP's num_members = %d (particle p follows "
                             "member p %% num_members: the members must carry equal weight)" % (p, len(members)))
        self._risk = (L.RISK_MEAN_STD, 0)
        if risk_alpha is not None:
            if float(risk_kappa) != 0.0:
                raise ValueError("risk_alpha (CVaR) and risk_kappa != 0 (mean - kappa * std) are two scoring rules: give one")
            self._risk = (L.RISK_CVAR, cvar_tail_count(risk_alpha, p))
        self._num_particles, self._process_noise_std, self._risk_kappa = p, sg, float(risk_kappa)
        if constraint is not None:
            if not (callable(getattr(constraint, "bounds", None)) and hasattr(constraint, "max_violation") and hasattr(constraint, "weight")):
                raise ValueError("constraint must be a StateBoxConstraint, got %r" % (constraint,))
            if getattr(system_dynamics_handler._dynamics_function, "_bbmpc_dynamics_kind", None) != L.DYN_MLP:
                raise NotImplementedError("a StateBoxConstraint is tested on the particle rollouts of a learned model "
                                          "(DeterministicMLP, EnsembleMLP, ProbabilisticMLP), not of %s"
                                          % type(system_dynamics_handler._dynamics_function).__name__)
            constraint.bounds(dim_s)                       # (a box of another length is refused here)
        self._constraint = constraint

    @property
    def risk_settings(self):
        """(kind, tail_count): what goes to Engine.set_particle_risk after set_particles."""
        return self._risk

    def quantile_ranks(self, quantiles):
        """Levels tau in (0, 1] -> nearest ranks among this evaluator's particles."""
        levels = np.asarray(quantiles, np.float64).reshape(-1)
        if not 1 <= levels.size <= L.MAX_QUANTILE_LEVELS:
            raise ValueError("quantiles must hold 1 to %d levels, got %d" % (L.MAX_QUANTILE_LEVELS, levels.size))
        return [quantile_rank(t, self._num_particles) for t in levels]

    @property
    def particle_settings(self):
        """(num_particles, process_noise_std [dim_S], risk_kappa): what OptimizerBase.set_trajectory_evaluator hands to
        Engine.set_particles."""
        return self._num_particles, self._process_noise_std, self._risk_kappa

    def _particle_engine(self, seq):
        if seq.ndim != 4:
            raise ValueError("action_sequences must be [population, num_agents, planning_horizon, dim_U]")
        return self._apply_particles(self._engine(seq.shape[1], seq.shape[2]))

    def _apply_particles(self, eng):
        """The particle settings on `eng` unless they are this evaluator's already."""
        if getattr(eng, "P", 0) != self._num_particles or getattr(eng, "_particle_settings", None) is not self:
            if getattr(eng, "risk", (L.RISK_MEAN_STD, 0))[1] > self._num_particles:
                eng.set_particle_risk(L.RISK_MEAN_STD, 0)      # another evaluator's tail would not fit these particles
            eng.set_particles(*self.particle_settings)
            eng.set_particle_risk(*self.risk_settings)         # (also resets a CVaR another evaluator left behind)
            eng._particle_settings = self
            eng.__dict__.pop("_constraint_version", None)       # (set_particles(0) in between would have removed the box)
        if constraint_stale(eng, self):
            configure_constraint(eng, self)
        return eng

    def _violations(self, current_states, action_sequences, first_steps):
        if self._constraint is None:
            raise ValueError("this ParticleTrajectoryEvaluator has no constraint (construct it with constraint=StateBoxConstraint(...))")
        seq = np.asarray(action_sequences, np.float32)
        eng = self._particle_engine(seq)
        eng.evaluate_particles(current_states, seq, want_returns=False)
        return eng.constraint_violations(seq.shape[0], first_steps=first_steps)

    def violation_probability(self, current_states, action_sequences):
        """current_states [A,S], action_sequences [N,A,H,U] -> v [N,A]: the share of each sequence's particles whose noisy
        state leaves the constraint's box at some step of the horizon."""
        return self._violations(current_states, action_sequences, False)

    def first_violation_steps(self, current_states, action_sequences):
        """... -> int32 [N,P,A]: per particle the first step in 1 .. H outside the box, 0 = never."""
        return self._violations(current_states, action_sequences, True)[1]

    def predict_trajectory_distribution(self, current_states, action_sequences, eps=None, return_particles=False, quantiles=None):
        """current_states [B,S], action_sequences [B,Hq,U] -> (state_mean [B,Hq,S], state_std [B,Hq,S], reward_mean [B,Hq],
        reward_std [B,Hq]) over the particles, each rolled open loop from the row's own start state with this evaluator's
        process noise -- and, with an EnsembleMLP / ProbabilisticMLP handler, the member it follows and the noise its head
        predicts; with return_particles also (particle_states [B,P,Hq,S], particle_rewards [B,P,Hq]).  eps: standard
        normals [B,P,Hq,S], or None for the engine's own draws.  quantiles: up to 8 levels tau in (0, 1], e.g. [0.05, 0.95] --
        then state_quantiles [B,L,Hq,S] and reward_quantiles [B,L,Hq] follow the four moments: for each level the particle
        value of nearest rank ceil(tau P) - 1 (an element of the particle tensor; a band a skewed distribution is plotted
        with).  Served by the one-step calls' engine, as predict_trajectories (Hq is free of any planning horizon)."""
        ranks = None if quantiles is None else self.quantile_ranks(quantiles)
        eng = self._apply_particles(self._engine(self._one_step_agents(), 1))
        return eng.predict_trajectory_particles(current_states, action_sequences, eps=eps, want_particles=return_particles,
                                                quantile_ranks=ranks)

    def __call__(self, current_states, action_sequences, time_step=0):
        """current_states [A,S], action_sequences [N,A,H,U] -> scores [N,A]."""
        seq = np.asarray(action_sequences, np.float32)
        return self._particle_engine(seq).evaluate(current_states, seq)

    def particle_returns(self, current_states, action_sequences):
        """The per-particle returns [N, P, A] behind the scores (NaN -> -1e6 per particle)."""
        seq = np.asarray(action_sequences, np.float32)
        return self._particle_engine(seq).evaluate_particles(current_states, seq)[1]
