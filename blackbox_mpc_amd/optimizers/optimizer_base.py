"""OptimizerBase -- the reference's optimizer interface (optimizers/optimizer_base.py:5-115).

A subclass only declares which engine optimizer it is and its hyper-parameters; the whole
per-control-step loop (sample -> rollout -> reduce -> refit, every iteration, plus the
exploration-noise / predicted-next-state tail of __call__) runs on the GPU through the C ABI."""
import numpy as np

from .. import _lib as L
from ..engine import Engine


class OptimizerBase:
    _engine_optimizer = L.OPT_NONE

    def __init__(self, name, planning_horizon, max_iterations, num_agents, env_action_space,
                 env_observation_space, seed=0, quirks=0, agent_offset=0, num_agents_global=None, device=-1,
                 population_offset=0, population_global=0):
        self.name = name
        self._planning_horizon = int(planning_horizon)
        self._env_action_space = env_action_space
        self._env_observation_space = env_observation_space
        self._dim_U = int(env_action_space.shape[0])
        self._dim_S = int(env_observation_space.shape[0])
        self._action_upper_bound = np.asarray(env_action_space.high, np.float32)
        self._action_lower_bound = np.asarray(env_action_space.low, np.float32)
        self._num_agents = int(num_agents)
        self._max_iterations = max_iterations
        self._trajectory_evaluator = None
        self._exploration_variance = (np.square(self._action_lower_bound - self._action_upper_bound) / 16) * 0.05
        self._exploration_mean = (self._action_upper_bound + self._action_lower_bound) / 2
        self._seed, self._quirks = int(seed), int(quirks)
        self._agent_offset, self._num_agents_global, self._device = int(agent_offset), num_agents_global, int(device)
        self._population_offset, self._population_global = int(population_offset), int(population_global or 0)
        self._engine = None

    # hyper-parameters forwarded to bbmpc_config; overridden by subclasses
    def _engine_kwargs(self):
        return {}

    def _optimize(self, current_state, time_step):
        raise Exception("__call__ function is not implemented yet")

    def _require_engine(self):
        if self._engine is None:
            if type(self)._engine_optimizer == L.OPT_NONE:
                raise Exception("__call__ function is not implemented yet")
            raise Exception("trajectory evaluator is not set; call set_trajectory_evaluator first")
        eng = self._engine
        h = self._trajectory_evaluator._system_dynamics_handler
        # inline staleness test (a learned model that was refitted / reloaded is re-uploaded before the next step)
        if eng.__dict__.get("_dyn_version") != (getattr(h._dynamics_function, "_version", 0), h._version):
            from ..trajectory_evaluators.deterministic import configure_dynamics
            configure_dynamics(eng, h)
        if eng.cfg.reward == L.REW_MLP:               # a learned reward model that was refitted / reloaded, likewise
            rf = self._trajectory_evaluator._reward_function
            if eng.__dict__.get("_rew_version") != getattr(rf, "_version", 0):
                from ..trajectory_evaluators.deterministic import configure_reward
                configure_reward(eng, rf)
        value = getattr(self._trajectory_evaluator, "_terminal_value", None)      # a refitted value network, likewise
        if value is not None and eng.__dict__.get("_val_version") != getattr(value, "_version", 0):
            from ..trajectory_evaluators.deterministic import configure_terminal_value
            configure_terminal_value(eng, self._trajectory_evaluator)
        term = getattr(self._trajectory_evaluator, "_termination", None)          # a box whose bounds were changed, likewise
        if term is not None and eng.__dict__.get("_shaping_version", (0, 0, 0))[2] != term._version:
            from ..trajectory_evaluators.deterministic import configure_return_shaping
            configure_return_shaping(eng, self._trajectory_evaluator)
        box = getattr(self._trajectory_evaluator, "_constraint", None)            # a chance constraint that was changed, likewise
        if box is not None and eng.__dict__.get("_constraint_version", (0, 0))[1] != box._version:
            from ..trajectory_evaluators.particle import configure_constraint
            configure_constraint(eng, self._trajectory_evaluator)
        prior = getattr(self, "_policy_prior", None)                              # a refitted policy prior, likewise
        if prior is not None and eng.__dict__.get("_prior_version") != getattr(prior[0], "_version", 0):
            self._configure_policy_prior(eng)
        return eng

    def _configure_policy_prior(self, eng):
        net, count, std = self._policy_prior
        if (net.dim_S, net.dim_U) != (self._dim_S, self._dim_U):
            raise ValueError("policy_prior maps %d -> %d but the optimizer's spaces are %d -> %d"
                             % (net.dim_S, net.dim_U, self._dim_S, self._dim_U))
        eng.set_policy_prior_mlp(net.weights, net.biases, net.activation_codes, stats=net.normalization_stats(), count=count,
                                 noise_std=std)
        eng._prior_version = getattr(net, "_version", 0)

    def _require_engine_and_params(self):
        # what _require_engine is on an optimizer whose reward / dynamics has runtime parameters: they are uploaded when
        # they changed since the last computation (set_trajectory_evaluator picks it, so built-ins skip the test)
        from ..utils.device_functions import sync_user_params
        eng = OptimizerBase._require_engine(self)
        sync_user_params(eng)
        return eng

    def __call__(self, current_state, time_step=0, add_exploration_noise=False):
        """(current_state[A,S], time_step, add_exploration_noise) ->
        (action[A,U], next_state[A,S], rewards_of_next_state[A])   optimizer_base.py:55-95"""
        return self._require_engine().optimize(current_state, time_step, add_exploration_noise)

    def keep_plan(self, enabled=True):
        """Switch plan readback on (off): control steps then take the paths that keep their solution in HBM -- same
        results, slower -- so that `plan` can read it.  Off by default."""
        self._require_engine().set_keep_plan(enabled)

    def plan(self, current_state):
        """(actions [A,H,U], states [A,H,S], rewards [A,H]): the solution the LAST __call__ took its action from (the final
        mean of CEM / PI2 / SPSA / CMA-ES, the best particle of RandomSearch / PSO), rolled out open loop from
        `current_state` through the model.  Needs keep_plan(True) before that call."""
        eng = self._require_engine()
        try:
            actions = eng.get_plan()
        except L.BBMPCError as ex:
            if ex.code == L.E_STATE:
                raise RuntimeError("plan(): plan readback was not on during the last call -- switch it on with "
                                   "optimizer.keep_plan(True) (MPCPolicy.keep_plan(True)) before calling the optimizer") from ex
            raise
        states, rewards = eng.predict_trajectories(np.asarray(current_state, np.float32), actions)
        return actions, states, rewards

    def plan_distribution(self, current_state, quantiles=None):
        """(actions [A,H,U], state_mean [A,H,S], state_std [A,H,S], reward_mean [A,H], reward_std [A,H]): the plan of
        `plan`, rolled out from `current_state` once per particle of the ParticleTrajectoryEvaluator -- process noise, the
        ensemble member a particle follows, the noise a log-variance head predicts -- and reduced to its per-step mean and
        spread.  quantiles: levels in (0, 1], e.g. [0.05, 0.95] -- then state_quantiles [A,L,H,S] and reward_quantiles
        [A,L,H] follow (ParticleTrajectoryEvaluator.predict_trajectory_distribution).  Needs keep_plan(True) before the call
        whose plan is wanted, and a ParticleTrajectoryEvaluator."""
        if getattr(self._trajectory_evaluator, "particle_settings", None) is None:
            raise TypeError("plan_distribution() needs a ParticleTrajectoryEvaluator (the optimizer's evaluator is %s, which is "
                            "deterministic: use plan())" % type(self._trajectory_evaluator).__name__)
        ranks = None if quantiles is None else self._trajectory_evaluator.quantile_ranks(quantiles)
        eng = self._require_engine()
        try:
            actions = eng.get_plan()
        except L.BBMPCError as ex:
            if ex.code == L.E_STATE:
                raise RuntimeError("plan_distribution(): plan readback was not on during the last call -- switch it on with "
                                   "optimizer.keep_plan(True) (MPCPolicy.keep_plan(True)) before calling the optimizer") from ex
            raise
        return (actions,) + eng.predict_trajectory_particles(np.asarray(current_state, np.float32), actions, quantile_ranks=ranks)

    def reset(self):
        if type(self)._engine_optimizer == L.OPT_NONE:
            raise Exception("reset function is not implemented yet")
        if self._engine is not None:
            self._engine.reset()

    def set_trajectory_evaluator(self, trajectory_evaluator):
        from ..trajectory_evaluators.deterministic import (configure_dynamics, configure_return_shaping, configure_reward,
                                                           configure_terminal_value, plugin_kinds, shaping_on)
        self._trajectory_evaluator = trajectory_evaluator
        if type(self)._engine_optimizer == L.OPT_NONE:
            return
        h = trajectory_evaluator._system_dynamics_handler
        dk, rk = plugin_kinds(trajectory_evaluator._reward_function, h)
        grad = getattr(self, "_grad_refine", None)    # CEM with grad_steps / grad_lr / grad_method / grad_candidates
        if grad is not None:
            df = h._dynamics_function
            if (dk != L.DYN_MLP or rk != L.REW_MLP or hasattr(df, "members") or getattr(df, "logvar_heads", None)
                    or getattr(trajectory_evaluator, "particle_settings", None) is not None):
                raise ValueError("grad_steps > 0 differentiates the candidates through learned networks: it needs learned dynamics "
                                 "(DeterministicMLP), a learned reward (LearnedRewardMLP) and the deterministic evaluator, got %s, %s "
                                 "and %s" % (type(df).__name__, type(trajectory_evaluator._reward_function).__name__,
                                             type(trajectory_evaluator).__name__))
        if grad is not None and shaping_on(trajectory_evaluator):
            raise ValueError("grad_steps > 0 beside discount / termination: the gradient steps climb the undiscounted return over the "
                             "full horizon, not the shaped one")
        if self._engine is not None:
            self._engine.close()
        quirks = self._quirks | int(getattr(trajectory_evaluator, "_quirks", 0))
        self._engine = Engine(type(self)._engine_optimizer, dk, rk, self._action_lower_bound, self._action_upper_bound,
                              dim_s=self._dim_S, num_agents=self._num_agents, planning_horizon=self._planning_horizon,
                              max_iterations=self._max_iterations or 0, seed=self._seed, quirks=quirks,
                              agent_offset=self._agent_offset, num_agents_global=self._num_agents_global,
                              device=self._device, population_offset=self._population_offset,
                              population_global=self._population_global, **self._engine_kwargs())
        configure_dynamics(self._engine, h)
        configure_reward(self._engine, trajectory_evaluator._reward_function)
        configure_terminal_value(self._engine, trajectory_evaluator)
        configure_return_shaping(self._engine, trajectory_evaluator)
        particles = getattr(trajectory_evaluator, "particle_settings", None)
        if particles is not None:                     # a ParticleTrajectoryEvaluator: (num_particles, process_noise_std, risk_kappa)
            self._engine.set_particles(*particles)
            risk = getattr(trajectory_evaluator, "risk_settings", (L.RISK_MEAN_STD, 0))
            if risk[0] != L.RISK_MEAN_STD:            # (the engine is new: mean - kappa * std is what it starts with)
                self._engine.set_particle_risk(*risk)
            from ..trajectory_evaluators.particle import configure_constraint
            configure_constraint(self._engine, trajectory_evaluator)      # a StateBoxConstraint (constraint=), behind set_particles
        mix = getattr(self, "_sampling_mix", None)    # CEM / PI2 with noise_beta / sampling_correlation
        if mix is not None:
            self._engine.set_sampling_correlation(mix)
        carry = getattr(self, "_elite_carry", (0, 0))  # CEM with keep_elites / shift_elites
        if carry != (0, 0):
            self._engine.set_elite_carry(*carry)
        if getattr(self, "_policy_prior", None) is not None:   # CEM with policy_prior / prior_candidates / prior_std
            self._configure_policy_prior(self._engine)
        if grad is not None:
            self._engine.set_grad_refine(*grad)
        if self._engine._param_fns:
            self._require_engine = self._require_engine_and_params
        else:
            self.__dict__.pop("_require_engine", None)
        return
