from .deterministic_mlp import DeterministicMLP  # noqa: F401
from .ensemble_mlp import EnsembleMLP  # noqa: F401
from .probabilistic_mlp import ProbabilisticMLP  # noqa: F401
