"""Cross-Entropy Method -- kwargs/defaults of the reference's CEMOptimizer (optimizers/cem.py:7-10)."""
from .. import _lib as L
from ..utils.colored_noise import resolve_sampling_correlation
from .optimizer_base import OptimizerBase


class CEMOptimizer(OptimizerBase):
    _engine_optimizer = L.OPT_CEM

    def __init__(self, env_action_space, env_observation_space, planning_horizon=50, max_iterations=5,
                 population_size=500, num_elite=50, num_agents=5, epsilon=0.001, alpha=0.25, noise_beta=None,
                 sampling_correlation=None, **engine_args):
        # temporally correlated sampling (no counterpart in the reference): noise_beta = the exponent of iCEM's colored
        # noise, or sampling_correlation = an [H, H] mixing matrix of the caller's (utils/colored_noise.py)
        self._sampling_mix = resolve_sampling_correlation(planning_horizon, noise_beta, sampling_correlation)
        super().__init__(name=None, planning_horizon=planning_horizon, max_iterations=max_iterations,
                         num_agents=num_agents, env_action_space=env_action_space,
                         env_observation_space=env_observation_space, **engine_args)
        self._population_size = int(population_size)
        self._num_elite = int(num_elite)
        self._epsilon = epsilon  # stored and never used, as in the reference (cem.py:53)
        self._alpha = float(alpha)

    def _engine_kwargs(self):
        return dict(population_size=self._population_size, num_elite=self._num_elite, alpha=self._alpha)
