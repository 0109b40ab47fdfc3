"""MPCPolicy -- drop-in for the reference's policies/mpc_policy.py:8-245.

Same constructor kwargs, `act / reset / switch_optimizer`, same error behaviour; one `act` is one
C-ABI call (state up, all optimizer iterations on the GPU, packed action/next-state/reward down)."""
import numpy as np

from ..dynamics_handlers.system_dynamics_handler import SystemDynamicsHandler
from ..trajectory_evaluators.deterministic import DeterministicTrajectoryEvaluator
from .model_based_base_policy import ModelBasedBasePolicy


def _optimizer_class(optimizer_name):
    from .. import optimizers as O
    return {"CEM": O.CEMOptimizer, "CMA-ES": O.CMAESOptimizer, "PI2": O.PI2Optimizer, "PSO": O.PSOOptimizer,
            "SPSA": O.SPSAOptimizer, "RandomSearch": O.RandomSearchOptimizer}.get(optimizer_name)


class MPCPolicy(ModelBasedBasePolicy):
    def __init__(self, trajectory_evaluator=None, optimizer=None, tf_writer=None, log_dir=None,
                 reward_function=None, env_action_space=None, env_observation_space=None,
                 dynamics_function=None, dynamics_handler=None, true_model=False, optimizer_name=None,
                 num_agents=None, save_model_frequency=1, saved_model_dir=None, terminal_value=None, terminal_weight=1.0,
                 refine_steps=0, refine_lr=0.05, refine_device=False, discount=1.0, termination=None, constraint=None, **optimizer_args):
        """constraint: the utils.constraints.StateBoxConstraint of the ParticleTrajectoryEvaluator passed in (it must carry
        this very object: a chance constraint is a statement about particles, and the evaluator this constructor builds is
        deterministic); `plan_violation` then reports the plan's violation probability.
        terminal_value / terminal_weight: a LearnedValueMLP that closes the planning horizon (handed to the
        DeterministicTrajectoryEvaluator this constructor builds; an evaluator passed in takes them itself).
        discount / termination: a discount in (0, 1] and a utils.termination.StateBoxTermination, handed to that evaluator
        likewise: plans score sum_t discount^t r_t up to the first state outside the box (bbmpc_set_return_shaping); not
        together with refine_steps or grad_steps, whose gradient is that of the unshaped return.
        refine_steps / refine_lr: with refine_steps > 0 every `act` refines the optimizer's plan by that many projected
        gradient steps on the model return (utils.plan_refinement.refine_plan, Engine.plan_gradient) and acts on the refined
        plan's first action; needs learned dynamics and a LearnedRewardMLP.  The optimizer's own warm start is left alone.
        refine_steps = 0 changes nothing.  refine_device=True runs those steps on the device (Engine.refine_plans: the same
        rule in float32, no host visit between steps); the default keeps the host loop.  grad_steps / grad_lr / grad_method /
        grad_candidates (optimizer_name="CEM") go to CEMOptimizer: gradient steps on the candidates of every iteration."""
        self._refine_steps, self._refine_lr = int(refine_steps), float(refine_lr)
        if not isinstance(refine_device, (bool, np.bool_)):
            raise ValueError("refine_device must be a bool, got %r" % (refine_device,))
        self._refine_device = bool(refine_device)
        if self._refine_steps < 0:
            raise ValueError("refine_steps must be >= 0, got %r" % (refine_steps,))
        if self._refine_steps > 0:
            if not (self._refine_lr > 0.0 and np.isfinite(self._refine_lr)):
                raise ValueError("refine_lr must be positive and finite, got %r" % (refine_lr,))
            from .. import _lib as L
            rf = reward_function if trajectory_evaluator is None else trajectory_evaluator._reward_function
            handler = dynamics_handler if trajectory_evaluator is None else trajectory_evaluator._system_dynamics_handler
            df = dynamics_function if handler is None else handler._dynamics_function
            if (getattr(rf, "_bbmpc_reward_kind", None) != L.REW_MLP or getattr(df, "_bbmpc_dynamics_kind", None) != L.DYN_MLP
                    or hasattr(df, "members") or getattr(df, "logvar_heads", None)):
                raise ValueError("refine_steps > 0 differentiates the plan through learned networks: it needs learned dynamics "
                                 "(DeterministicMLP) and a learned reward (LearnedRewardMLP), got %s and %s"
                                 % (type(df).__name__, type(rf).__name__))
        self._refined_plan = self._unrefined_plan = None
        if constraint is not None and (trajectory_evaluator is None or getattr(trajectory_evaluator, "particle_settings", None) is None
                                       or getattr(trajectory_evaluator, "_constraint", None) is not constraint):
            raise ValueError("constraint needs a ParticleTrajectoryEvaluator that carries it: construct "
                             "ParticleTrajectoryEvaluator(..., constraint=constraint) and pass it as trajectory_evaluator (the "
                             "evaluator MPCPolicy builds itself is deterministic and has no particles)")
        if trajectory_evaluator is not None and terminal_value is not None:
            raise ValueError("terminal_value goes to the trajectory evaluator: construct it with terminal_value=, "
                             "or leave trajectory_evaluator to MPCPolicy")
        if trajectory_evaluator is not None and (termination is not None or float(discount) != 1.0):
            raise ValueError("discount / termination go to the trajectory evaluator: construct it with discount=, termination=, "
                             "or leave trajectory_evaluator to MPCPolicy")
        from ..trajectory_evaluators.deterministic import shaping_on
        shaped = (termination is not None or float(discount) != 1.0) if trajectory_evaluator is None else shaping_on(trajectory_evaluator)
        if shaped and (self._refine_steps > 0 or int(optimizer_args.get("grad_steps", 0) or 0) > 0):
            raise ValueError("refine_steps / grad_steps beside discount / termination: the gradient is that of the undiscounted "
                             "return over the full horizon, not of the shaped one")
        if trajectory_evaluator is None:
            if dynamics_handler is None:
                dynamics_handler = SystemDynamicsHandler(
                    env_action_space=env_action_space, env_observation_space=env_observation_space,
                    true_model=true_model, dynamics_function=dynamics_function, log_dir=log_dir,
                    tf_writer=tf_writer, save_model_frequency=save_model_frequency,
                    saved_model_dir=saved_model_dir)
            trajectory_evaluator = DeterministicTrajectoryEvaluator(reward_function=reward_function,
                                                                    system_dynamics_handler=dynamics_handler,
                                                                    terminal_value=terminal_value,
                                                                    terminal_weight=terminal_weight,
                                                                    discount=discount, termination=termination)
        super(MPCPolicy, self).__init__(trajectory_evaluator=trajectory_evaluator)
        if optimizer is None:
            if num_agents is None:
                raise Exception("Please Specify Num Of Agents in the MPC")
            cls = _optimizer_class(optimizer_name)
            if cls is not None:
                optimizer = cls(env_action_space=env_action_space, env_observation_space=env_observation_space,
                                num_agents=num_agents, **optimizer_args)
        self._optimizer = optimizer
        self._tf_writer = tf_writer
        self._trajectory_evaluator = trajectory_evaluator
        # an unknown optimizer_name leaves optimizer None -> AttributeError here, as in the reference (:120)
        self._optimizer.set_trajectory_evaluator(trajectory_evaluator)
        self._act_call_counter = 0

    def act(self, observations, t, exploration_noise=False):
        observations = np.asarray(observations)
        batched = observations
        if observations.ndim == 1:
            batched = np.tile(observations[None], (self._optimizer._num_agents, 1))
        if self._refine_steps > 0:
            if exploration_noise:
                raise ValueError("exploration noise and plan refinement in one call: the refined action is the plan's first "
                                 "action (construct the policy with refine_steps=0 to explore)")
            action, next_observations, rewards = self._act_refined(batched, t)
        else:
            action, next_observations, rewards = self._optimizer(batched, t, exploration_noise)
        self._act_call_counter += 1
        if observations.ndim == 1:
            return action[0], next_observations[0], rewards[0]
        return action, next_observations, rewards

    def _act_refined(self, batched, t):
        """The optimizer's control step, then refine_steps projected gradient steps on its plan: (first action of the
        refined plan [A,U], the model's next state [A,S] and reward [A] for that action)."""
        from ..utils.plan_refinement import refine_plan
        opt = self._optimizer
        if not getattr(self, "_refine_readback_on", False) or opt._engine is not getattr(self, "_refine_engine", None):
            opt.keep_plan(True)
            self._refine_readback_on, self._refine_engine = True, opt._engine
        opt(batched, t, False)
        eng = opt._require_engine()
        plan = eng.get_plan()
        if self._refine_device:
            refined, ret = eng.refine_plans(np.asarray(batched, np.float32), plan, self._refine_steps, self._refine_lr)
        else:
            refined, ret = refine_plan(eng, np.asarray(batched, np.float32), plan, self._refine_steps, self._refine_lr,
                                       opt._action_lower_bound, opt._action_upper_bound)
        self._unrefined_plan, self._refined_plan, self._refined_return = plan, refined, ret
        states, rewards = eng.predict_trajectories(np.asarray(batched, np.float32), refined[:, :1])
        return refined[:, 0].copy(), states[:, 0], rewards[:, 0]

    def keep_plan(self, enabled=True):
        """Switch plan readback on (off) for the `act` calls that follow (OptimizerBase.keep_plan)."""
        self._optimizer.keep_plan(enabled)

    def plan(self, observations):
        """The plan the last `act` took its action from, rolled out from `observations`: (actions [A,H,U], states [A,H,S],
        rewards [A,H]); a 1-D observation is un-batched as in `act` ([H,U], [H,S], [H])."""
        observations = np.asarray(observations)
        batched = observations
        if observations.ndim == 1:
            batched = np.tile(observations[None], (self._optimizer._num_agents, 1))
        if self._refine_steps > 0:                      # the refined plan the last `act` acted on
            if self._refined_plan is None:
                raise RuntimeError("plan(): call act() first")
            actions = self._refined_plan
            states, rewards = self._optimizer._require_engine().predict_trajectories(np.asarray(batched, np.float32), actions)
        else:
            actions, states, rewards = self._optimizer.plan(batched)
        if observations.ndim == 1:
            return actions[0], states[0], rewards[0]
        return actions, states, rewards

    def plan_distribution(self, observations, quantiles=None):
        """The plan the last `act` took its action from, rolled out from `observations` once per particle of the
        ParticleTrajectoryEvaluator: (actions [A,H,U], state_mean [A,H,S], state_std [A,H,S], reward_mean [A,H],
        reward_std [A,H]) and, with quantile levels such as [0.05, 0.95], (state_quantiles [A,L,H,S], reward_quantiles
        [A,L,H]); a 1-D observation is un-batched as in `plan`."""
        observations = np.asarray(observations)
        batched = observations
        if observations.ndim == 1:
            batched = np.tile(observations[None], (self._optimizer._num_agents, 1))
        out = self._optimizer.plan_distribution(batched, quantiles=quantiles)
        if observations.ndim == 1:
            return tuple(o[0] for o in out)
        return out

    def plan_violation(self, observations):
        """v [A] of the plan the last `act` took its action from (a scalar for a 1-D observation): the share of the
        ParticleTrajectoryEvaluator's particles that leave its StateBoxConstraint when the plan is rolled out from
        `observations` (violation_probability of the plan `plan` returns).  Needs keep_plan(True) before that `act`."""
        ev = self._trajectory_evaluator
        if getattr(ev, "_constraint", None) is None:
            raise ValueError("plan_violation() needs a ParticleTrajectoryEvaluator constructed with constraint=")
        observations = np.asarray(observations)
        batched = observations
        if observations.ndim == 1:
            batched = np.tile(observations[None], (self._optimizer._num_agents, 1))
        actions = self._optimizer.plan(batched)[0]
        v = ev.violation_probability(np.asarray(batched, np.float32), actions[None])[0]
        return v[0] if observations.ndim == 1 else v

    def reset(self):
        self._optimizer.reset()

    def switch_optimizer(self, optimizer=None, optimizer_name='', **optimizer_args):
        if optimizer is None:
            cls = _optimizer_class(optimizer_name)
            if cls is not None:
                old = self._optimizer
                self._optimizer = cls(env_action_space=old._env_action_space,
                                      env_observation_space=old._env_observation_space,
                                      num_agents=old._num_agents, **optimizer_args)
        else:
            self._optimizer = optimizer
        self._optimizer.set_trajectory_evaluator(self._trajectory_evaluator)
        return
