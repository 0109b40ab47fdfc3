from .deterministic_mlp import DeterministicMLP  # noqa: F401
from .ensemble_mlp import EnsembleMLP  # noqa: F401
