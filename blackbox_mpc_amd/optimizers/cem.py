"""Cross-Entropy Method -- kwargs/defaults of the reference's CEMOptimizer (optimizers/cem.py:7-10)."""
import numbers

from .. import _lib as L
from ..utils.colored_noise import resolve_sampling_correlation
from .optimizer_base import OptimizerBase


def _elite_count(name, value, num_elite):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral):
        raise ValueError("%s must be an int, got %r" % (name, value))
    if value < 0 or value > int(num_elite):
        raise ValueError("%s must lie in [0, num_elite] = [0, %d], got %d" % (name, int(num_elite), value))
    return int(value)


def _policy_prior_setting(policy_prior, prior_candidates, prior_std, carry, population_size):
    """(network, count, std), or None without a network."""
    if isinstance(prior_candidates, bool) or not isinstance(prior_candidates, numbers.Integral):
        raise ValueError("prior_candidates must be an int, got %r" % (prior_candidates,))
    if isinstance(prior_std, bool) or not isinstance(prior_std, numbers.Real) or not (0.0 <= float(prior_std) < float("inf")):
        raise ValueError("prior_std must be a finite number >= 0, got %r" % (prior_std,))
    if policy_prior is None:
        if prior_candidates != 0:
            raise ValueError("prior_candidates = %d without a policy_prior network" % prior_candidates)
        return None
    for attr in ("weights", "biases", "activation_codes", "normalization_stats"):
        if not hasattr(policy_prior, attr):
            raise TypeError("policy_prior must be a LearnedPolicyMLP (an object with weights, biases, activation_codes and "
                            "normalization_stats()), got %s" % type(policy_prior).__name__)
    if prior_candidates < 1:
        raise ValueError("prior_candidates must be >= 1 with a policy_prior network, got %d" % prior_candidates)
    if prior_candidates + max(carry) >= int(population_size):
        raise ValueError("prior_candidates + max(keep_elites, shift_elites) = %d must be below population_size = %d"
                         % (prior_candidates + max(carry), int(population_size)))
    return policy_prior, int(prior_candidates), float(prior_std)


def _grad_refine_setting(grad_steps, grad_lr, grad_method, grad_candidates, population_size):
    """(steps, lr, method, candidates), or None with grad_steps = 0."""
    for name, value in (("grad_steps", grad_steps), ("grad_candidates", grad_candidates)):
        if isinstance(value, bool) or not isinstance(value, numbers.Integral):
            raise ValueError("%s must be an int, got %r" % (name, value))
    if grad_steps < 0 or grad_steps > 64:
        raise ValueError("grad_steps must lie in [0, 64], got %d" % grad_steps)
    if grad_candidates < 0 or grad_candidates > int(population_size):
        raise ValueError("grad_candidates must lie in [0, population_size] = [0, %d] (0: all), got %d"
                         % (int(population_size), grad_candidates))
    if isinstance(grad_lr, bool) or not isinstance(grad_lr, numbers.Real) or not (0.0 < float(grad_lr) < float("inf")):
        raise ValueError("grad_lr must be a finite number > 0, got %r" % (grad_lr,))
    if grad_method not in ("adam", "sgd"):
        raise ValueError("grad_method must be 'adam' or 'sgd', got %r" % (grad_method,))
    if grad_steps == 0:
        return None
    return int(grad_steps), float(grad_lr), grad_method, int(grad_candidates)


class CEMOptimizer(OptimizerBase):
    _engine_optimizer = L.OPT_CEM

    def __init__(self, env_action_space, env_observation_space, planning_horizon=50, max_iterations=5,
                 population_size=500, num_elite=50, num_agents=5, epsilon=0.001, alpha=0.25, noise_beta=None,
                 sampling_correlation=None, keep_elites=0, shift_elites=0, policy_prior=None, prior_candidates=0,
                 prior_std=0.0, grad_steps=0, grad_lr=0.05, grad_method="adam", grad_candidates=0, **engine_args):
        # temporally correlated sampling (no counterpart in the reference): noise_beta = the exponent of iCEM's colored
        # noise, or sampling_correlation = an [H, H] mixing matrix of the caller's (utils/colored_noise.py)
        self._sampling_mix = resolve_sampling_correlation(planning_horizon, noise_beta, sampling_correlation)
        # elite carry-over, the other half of iCEM (Engine.set_elite_carry): the best keep_elites of an iteration are put
        # back among the candidates of the next one, the best shift_elites of a control step, moved one planning step
        # forward, among those of the next control step
        self._elite_carry = (_elite_count("keep_elites", keep_elites, num_elite), _elite_count("shift_elites", shift_elites, num_elite))
        # learned policy prior (Engine.set_policy_prior_mlp): prior_candidates closed-loop rollouts of policy_prior (a
        # LearnedPolicyMLP) through the learned model, with N(0, prior_std^2) on every action, replace that many sampled
        # candidates of every iteration
        self._policy_prior = _policy_prior_setting(policy_prior, prior_candidates, prior_std, self._elite_carry, population_size)
        # gradient steps on the candidates of every iteration (GradCEM; Engine.set_grad_refine): the last grad_candidates
        # columns (0: all) take grad_steps Adam / SGD steps on the model return before the rollout scores them; needs learned
        # dynamics, a LearnedRewardMLP and the deterministic evaluator (checked when the evaluator is set)
        self._grad_refine = _grad_refine_setting(grad_steps, grad_lr, grad_method, grad_candidates, population_size)
        super().__init__(name=None, planning_horizon=planning_horizon, max_iterations=max_iterations,
                         num_agents=num_agents, env_action_space=env_action_space,
                         env_observation_space=env_observation_space, **engine_args)
        self._population_size = int(population_size)
        self._num_elite = int(num_elite)
        self._epsilon = epsilon  # stored and never used, as in the reference (cem.py:53)
        self._alpha = float(alpha)

    def _engine_kwargs(self):
        return dict(population_size=self._population_size, num_elite=self._num_elite, alpha=self._alpha)
