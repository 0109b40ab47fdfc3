from .learned_value_mlp import LearnedValueMLP, value_targets  # noqa: F401
