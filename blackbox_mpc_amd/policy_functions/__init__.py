from .learned_policy_mlp import LearnedPolicyMLP  # noqa: F401
