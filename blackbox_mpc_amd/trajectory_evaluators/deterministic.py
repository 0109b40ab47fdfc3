"""DeterministicTrajectoryEvaluator -- same interface as the reference's
(trajectory_evaluators/deterministic.py:5-127), backed by the HIP rollout kernels."""
import numpy as np

from .. import _lib as L
from ..engine import Engine
from .evaluator_base import EvaluatorBase


_REWARD_HELP = (
    "reward_function %r cannot run on the GPU: rollouts never leave it, so a custom reward is either device code -- HIP "
    "source wrapped in blackbox_mpc_amd.utils.device_functions.HipRewardFunction (or any object with a `hip_source` "
    "attribute) -- or a callable that works on PyTorch CUDA tensors, reward(current_state[B,S], actions[B,U], "
    "next_state[B,S]) -> [B] (%s).  Built-ins: blackbox_mpc_amd.utils.pendulum.pendulum_reward_function, "
    "blackbox_mpc_amd.utils.cheetah.reward_function")
_DYNAMICS_HELP = (
    "dynamics_function %r cannot run on the GPU: a custom model is either device code -- HIP source wrapped in "
    "blackbox_mpc_amd.utils.device_functions.HipDynamicsFunction -- or a callable / torch.nn.Module that works on "
    "PyTorch CUDA tensors, f(x[B,S+U]) -> [B,S] (%s).  Built-ins: PendulumTrueModel, DeterministicMLP")


def reward_plugin(reward_function, handler):
    """The object the engine is configured from: the function itself when it is a built-in or carries HIP source, else
    (a plain callable, what the reference's users pass, deterministic.py:13-18) its torch adapter -- probed once on a
    two-row batch of CUDA tensors, so that a host-only function is refused here and not in the middle of a control step."""
    from ..utils import device_functions as DF
    if getattr(reward_function, "_bbmpc_reward_kind", None) is not None or isinstance(getattr(reward_function, "hip_source", None), str):
        return reward_function
    if not callable(reward_function):
        raise NotImplementedError(_REWARD_HELP % (reward_function, "it is not callable"))
    dev = DF.gpu_for_callables()
    if dev is None:
        raise NotImplementedError(_REWARD_HELP % (reward_function, "no GPU / PyTorch here to run it on"))
    plug = DF.torch_plugin(reward_function, DF.TorchRewardFunction)
    try:
        plug.probe(handler._dim_S, handler._dim_U, dev)
    except Exception as ex:                               # noqa: BLE001
        raise NotImplementedError(_REWARD_HELP % (reward_function, "calling it with CUDA tensors failed: %s: %s"
                                                  % (type(ex).__name__, ex))) from ex
    return plug


def dynamics_plugin(handler):
    from ..utils import device_functions as DF
    dyn = handler._dynamics_function
    if getattr(dyn, "_bbmpc_dynamics_kind", None) is not None or isinstance(getattr(dyn, "hip_source", None), str):
        inverse = getattr(handler, "_inverse_transform_targets_func", None)
        if inverse is not None:
            if not isinstance(inverse, DF.HipInverseTargetTransform):
                raise NotImplementedError(
                    "inverse_transform_targets_func %r cannot run inside the built-in / HIP-source models' kernels: give it as "
                    "HIP source wrapped in blackbox_mpc_amd.utils.device_functions.HipInverseTargetTransform, or use a "
                    "dynamics_function that runs on PyTorch CUDA tensors" % (inverse,))
            if getattr(dyn, "_bbmpc_dynamics_kind", None) == L.DYN_PENDULUM:
                raise NotImplementedError("inverse_transform_targets_func: PendulumTrueModel keeps the default next = delta + "
                                          "state (HipInverseTargetTransform works with DeterministicMLP and HipDynamicsFunction)")
        return dyn
    if not callable(dyn):
        raise NotImplementedError(_DYNAMICS_HELP % (dyn, "it is not callable"))
    dev = DF.gpu_for_callables()
    if dev is None:
        raise NotImplementedError(_DYNAMICS_HELP % (dyn, "no GPU / PyTorch here to run it on"))
    plug = DF.torch_plugin(dyn, DF.TorchDynamicsFunction)
    try:
        plug.probe(handler, dev)
    except Exception as ex:                               # noqa: BLE001
        raise NotImplementedError(_DYNAMICS_HELP % (dyn, "calling it with CUDA tensors failed: %s: %s"
                                                    % (type(ex).__name__, ex))) from ex
    return plug


def plugin_kinds(reward_function, handler):
    """Map the user-supplied callables to the engine's plug-in kinds: built-in device functors, HIP
    source (BBMPC_*_USER, fused), or callables on torch CUDA tensors (BBMPC_*_USER with a device-memory callback)."""
    rp = reward_plugin(reward_function, handler)
    rk = getattr(rp, "_bbmpc_reward_kind", None)
    if rk is None:
        rk = L.REW_USER                       # any object that carries HIP source for bbmpc_user_reward
    dp = dynamics_plugin(handler)
    dk = getattr(dp, "_bbmpc_dynamics_kind", None)
    if dk is None:
        dk = L.DYN_USER
    if rk == L.REW_MLP and (dk != L.DYN_MLP or getattr(handler, "_inverse_transform_targets_func", None) is not None):
        raise NotImplementedError("a LearnedRewardMLP scores the rollouts of a learned model: it needs a DeterministicMLP (or "
                                  "EnsembleMLP / ProbabilisticMLP) dynamics function without an inverse target transform, not %s"
                                  % type(dp).__name__)
    hip_true_model = dk == L.DYN_PENDULUM or (dk == L.DYN_USER and isinstance(getattr(dp, "hip_source", None), str))
    if hip_true_model and not handler._is_true_model:
        raise Exception("%s must be used with true_model=True" % type(dp).__name__)
    return dk, rk


def configure_transform(engine, handler, dyn):
    """Attach the handler's HipInverseTargetTransform (built-in learned model / HIP-source true model), once per engine."""
    if getattr(dyn, "_bbmpc_dynamics_kind", None) != L.DYN_MLP and not isinstance(getattr(dyn, "hip_source", None), str):
        return
    inverse = getattr(handler, "_inverse_transform_targets_func", None)
    src = getattr(inverse, "hip_source", None)
    if getattr(engine, "_xform_source", None) is not src:
        engine.set_inverse_transform_source(src)
        engine._xform_source = src


def configure_dynamics(engine, handler):
    """Upload MLP weights + normalisation statistics when the dynamics are learned; attach user dynamics."""
    from ..utils import device_functions as DF
    dyn = dynamics_plugin(handler)
    configure_transform(engine, handler, dyn)
    if getattr(dyn, "_bbmpc_dynamics_kind", None) == L.DYN_MLP:
        engine.set_mlp(dyn.weights, dyn.biases, dyn.activation_codes, handler.normalization_stats())
        if hasattr(dyn, "members"):                   # an EnsembleMLP: member 0 above, all members for the particle rollouts
            engine.set_mlp_ensemble(dyn.members)
        if getattr(dyn, "logvar_heads", None):        # a ProbabilisticMLP / probabilistic EnsembleMLP: the heads come last
            engine.set_mlp_logvar_head(dyn.logvar_heads, dyn.min_logvar, dyn.max_logvar)
    elif engine.cfg.dynamics == L.DYN_USER and isinstance(getattr(dyn, "hip_source", None), str):
        np_ = getattr(dyn, "num_params", 0)
        if getattr(engine, "_dyn_source", None) is not dyn.hip_source or getattr(engine, "_dyn_nparams", 0) != np_:
            engine.set_dynamics_source(dyn.hip_source, np_)
            engine._dyn_source, engine._dyn_nparams = dyn.hip_source, np_
            DF.attach_params(engine, L.USER_KIND_DYNAMICS, dyn)
    elif engine.cfg.dynamics == L.DYN_USER:
        # a callable on torch CUDA tensors: rebuilt whenever the handler's statistics change (they are baked into it)
        engine.set_dynamics_callback(dyn.make_callback(handler, engine.device))
    engine._dyn_version = (getattr(handler._dynamics_function, "_version", 0), handler._version)


def configure_reward(engine, reward_function, handler=None):
    """Compile + attach the user's reward device function (or its torch callback), once per engine."""
    if engine.cfg.reward == L.REW_MLP:                # a LearnedRewardMLP: uploaded now and again whenever it was refitted / reloaded
        engine.set_reward_mlp(reward_function.weights, reward_function.biases, reward_function.activation_codes,
                              reward_function.input_mask, reward_function.normalization_stats())
        engine._rew_version = getattr(reward_function, "_version", 0)
        return
    if engine.cfg.reward != L.REW_USER:
        return
    from ..utils import device_functions as DF
    if isinstance(getattr(reward_function, "hip_source", None), str):
        np_ = getattr(reward_function, "num_params", 0)
        if getattr(engine, "_rew_source", None) is not reward_function.hip_source or getattr(engine, "_rew_nparams", 0) != np_:
            engine.set_reward_source(reward_function.hip_source, np_)
            engine._rew_source, engine._rew_nparams = reward_function.hip_source, np_
            DF.attach_params(engine, L.USER_KIND_REWARD, reward_function)
        return
    plug = reward_function if isinstance(reward_function, DF.TorchRewardFunction) else DF.torch_plugin(reward_function, DF.TorchRewardFunction)
    if getattr(engine, "_rew_plugin", None) is not plug:
        engine.set_reward_callback(plug.make_callback(engine.S, engine.U, engine.device))
        engine._rew_plugin = plug


def dynamics_stale(engine, handler):
    dyn = handler._dynamics_function
    return getattr(engine, "_dyn_version", None) != (getattr(dyn, "_version", 0), handler._version)


def reward_stale(engine, reward_function):
    """A learned reward model (REW_MLP) whose weights changed since they were uploaded; never true for the other kinds."""
    return engine.cfg.reward == L.REW_MLP and engine.__dict__.get("_rew_version") != getattr(reward_function, "_version", 0)


def configure_terminal_value(engine, evaluator):
    """Upload the evaluator's LearnedValueMLP (terminal_value=) and its weight; nothing to do without one."""
    value = getattr(evaluator, "_terminal_value", None)
    if value is None:
        return
    engine.set_terminal_value_mlp(value.weights, value.biases, value.activation_codes, value.normalization_stats(),
                                  evaluator._terminal_weight)
    engine._val_version = getattr(value, "_version", 0)


def terminal_value_stale(engine, evaluator):
    """A value network whose weights changed since they were uploaded (or that was never uploaded to this engine)."""
    value = getattr(evaluator, "_terminal_value", None)
    return value is not None and engine.__dict__.get("_val_version") != getattr(value, "_version", 0)


def shaping_on(evaluator):
    """Whether the evaluator shapes its returns: a discount below 1 or a termination (discount=, termination=)."""
    return getattr(evaluator, "_termination", None) is not None or getattr(evaluator, "_discount", 1.0) != 1.0


def _shaping_version(evaluator):
    term = getattr(evaluator, "_termination", None)
    return (getattr(evaluator, "_discount", 1.0), id(term), getattr(term, "_version", 0))


def configure_return_shaping(engine, evaluator):
    """Upload the evaluator's discount and StateBoxTermination (discount=, termination=); nothing to do without either."""
    if not shaping_on(evaluator):
        return
    term = evaluator._termination
    if term is None:
        engine.set_return_shaping(evaluator._discount)
    else:
        lo, hi = term.bounds(engine.S)
        engine.set_return_shaping(evaluator._discount, lo, hi, term.terminal_reward)
    engine._shaping_version = _shaping_version(evaluator)


def return_shaping_stale(engine, evaluator):
    """A box whose bounds or terminal reward changed since they were uploaded (or that was never uploaded to this engine)."""
    return shaping_on(evaluator) and engine.__dict__.get("_shaping_version") != _shaping_version(evaluator)


_SHAPED_GRADIENT = ("%s beside discount / termination: the differentiated return is the undiscounted sum over the full "
                    "horizon, not the shaped one (construct the evaluator with discount=1.0, termination=None)")


class DeterministicTrajectoryEvaluator(EvaluatorBase):
    def __init__(self, reward_function, system_dynamics_handler, quirks=0, terminal_value=None, terminal_weight=1.0,
                 discount=1.0, termination=None, constraint=None):
        """constraint: refused here -- a utils.constraints.StateBoxConstraint is a statement about the particles of
        ParticleTrajectoryEvaluator.
        terminal_value: a LearnedValueMLP V -- candidates then score sum_t r_t + terminal_weight * V(s_H) (learned
        dynamics only; bbmpc_set_terminal_value_mlp).  The one-step calls and predict_trajectories do not read it.
        discount in (0, 1] / termination: a utils.termination.StateBoxTermination -- candidates then score
        sum_t discount^t r_t up to the first state outside the box, where they collect discount^T * terminal_reward and no
        terminal value; candidates that stay inside close with discount^H * terminal_weight * V(s_H) (learned dynamics with
        a built-in reward or a LearnedRewardMLP; bbmpc_set_return_shaping)."""
        if constraint is not None:
            raise NotImplementedError("DeterministicTrajectoryEvaluator has no chance constraint: a StateBoxConstraint limits the share "
                                      "of PARTICLES that leave the box, and one noise-free rollout has none (use "
                                      "ParticleTrajectoryEvaluator(..., constraint=))")
        super().__init__(reward_function=reward_function, system_dynamics_handler=system_dynamics_handler, name=None)
        self._quirks = int(quirks)
        self._terminal_value = terminal_value
        self._terminal_weight = float(terminal_weight)
        if terminal_value is not None and not np.isfinite(self._terminal_weight):
            raise ValueError("terminal_weight must be finite")
        self._discount = float(discount)
        if not (np.isfinite(self._discount) and 0.0 < self._discount <= 1.0):
            raise ValueError("discount must lie in (0, 1], got %r" % (discount,))
        if termination is not None and not (callable(getattr(termination, "bounds", None)) and hasattr(termination, "terminal_reward")):
            raise ValueError("termination must be a StateBoxTermination, got %r" % (termination,))
        self._termination = termination
        self._engines = {}

    def _engine(self, num_agents, horizon):
        h = self._system_dynamics_handler
        key = (int(num_agents), int(horizon))
        eng = self._engines.get(key)
        if eng is None:
            dk, rk = plugin_kinds(self._reward_function, h)
            space = h._env_action_space
            eng = Engine(L.OPT_NONE, dk, rk, space.low, space.high, dim_s=h._dim_S, num_agents=key[0],
                         planning_horizon=key[1], quirks=self._quirks)
            configure_reward(eng, self._reward_function)
            self._engines[key] = eng
        if dynamics_stale(eng, h):
            configure_dynamics(eng, h)
        if reward_stale(eng, self._reward_function):
            configure_reward(eng, self._reward_function)
        if terminal_value_stale(eng, self):
            configure_terminal_value(eng, self)
        if return_shaping_stale(eng, self):
            configure_return_shaping(eng, self)
        if eng._param_fns:
            from ..utils.device_functions import sync_user_params
            sync_user_params(eng)
        return eng

    def _one_step_agents(self):
        """Agents of the one-step calls' engine: the rows of per-agent runtime parameters (B / A consecutive rows of a
        call belong to one agent), else 1."""
        for fn in (self._reward_function, self._system_dynamics_handler._dynamics_function):
            p = getattr(fn, "_params", None)
            if p is not None and p.ndim == 2:
                return p.shape[0]
        return 1

    def __call__(self, current_states, action_sequences, time_step=0):
        """current_states [A,S], action_sequences [N,A,H,U] -> rewards [N,A] (NaN -> -1e6)."""
        seq = np.asarray(action_sequences, np.float32)
        if seq.ndim != 4:
            raise ValueError("action_sequences must be [population, num_agents, planning_horizon, dim_U]")
        return self._engine(seq.shape[1], seq.shape[2]).evaluate(current_states, seq)

    def predict_next_state(self, current_states, current_actions):
        s = np.asarray(current_states, np.float32)
        return self._engine(self._one_step_agents(), 1).predict_next_state(s, np.asarray(current_actions, np.float32))

    def predict_trajectories(self, current_states, action_sequences):
        """current_states [B,S], action_sequences [B,Hq,U] -> (states [B,Hq,S], rewards [B,Hq]): predict_next_state and
        evaluate_next_reward composed Hq times from each row's own start state (open loop, actions as given).  Served by
        the one-step calls' engine -- the call's horizon is free of any planning horizon -- through the same staleness /
        parameter-sync logic as __call__."""
        return self._engine(self._one_step_agents(), 1).predict_trajectories(current_states, action_sequences)

    def value_and_gradient(self, current_states, action_sequences):
        """current_states [A,S], action_sequences [n,A,H,U] -> (rewards [n,A], grad [n,A,H,U]): the model return of every
        sequence -- sum_t r_t + terminal_weight * V(s_H), actions as given, no NaN rule -- and its derivative in every
        action (Engine.plan_gradient).  Needs learned dynamics and a LearnedRewardMLP.  Refitted networks are uploaded
        first, as in __call__."""
        if shaping_on(self):
            raise ValueError(_SHAPED_GRADIENT % "value_and_gradient")
        seq = np.asarray(action_sequences, np.float32)
        if seq.ndim != 4:
            raise ValueError("action_sequences must be [n, num_agents, planning_horizon, dim_U]")
        n, a, hq, u = seq.shape
        s = np.asarray(current_states, np.float32)
        if s.shape != (a, self._system_dynamics_handler._dim_S):
            raise ValueError("current_states must be [num_agents, dim_S]")
        rows = np.broadcast_to(s[None], (n, a, s.shape[1])).reshape(n * a, -1)
        ret, grad = self._engine(a, hq).plan_gradient(rows, seq.reshape(n * a, hq, u))
        return ret.reshape(n, a), grad.reshape(n, a, hq, u)

    def refine_plans_rows(self, states, plans, steps, lr, method="adam"):
        """states [B,S], plans [B,Hq,U] -> (plans [B,Hq,U], returns [B]): Engine.refine_plans (keep-best, the engine's own
        action bounds) on the engine value_and_gradient uses, so that refitted networks are uploaded first."""
        if shaping_on(self):
            raise ValueError(_SHAPED_GRADIENT % "refine_plans_rows")
        plans = np.asarray(plans, np.float32)
        if plans.ndim != 3:
            raise ValueError("plans must be [B, planning_horizon, dim_U]")
        return self._engine(self._one_step_agents(), 1).refine_plans(states, plans, steps, lr, method=method, keep_best=True)

    def evaluate_next_reward(self, current_states, next_states, current_actions):
        return self._engine(self._one_step_agents(), 1).evaluate_next_reward(current_states, next_states, current_actions)
