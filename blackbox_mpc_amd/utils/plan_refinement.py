"""First-order refinement of sampled plans through the learned model: projected gradient ascent on
the model return R = sum_t r(s_t, a_t, s_{t+1}) + w V(s_H), with the gradient of Engine.plan_gradient
(bbmpc_plan_gradient: one kernel launch per step for the whole batch of plans)."""
import numpy as np


def _backend(obj):
    """(states [B,S], plans [B,H,U]) -> (returns [B], grad [B,H,U]) from an Engine (plan_gradient) or from a
    DeterministicTrajectoryEvaluator (value_and_gradient, plans as n = 1 sequences of B agents)."""
    if hasattr(obj, "plan_gradient"):
        def call(states, plans):
            ret, grad = obj.plan_gradient(states, plans)
            return np.asarray(ret, np.float64), np.asarray(grad, np.float64)
        return call
    if hasattr(obj, "value_and_gradient"):
        def call(states, plans):
            ret, grad = obj.value_and_gradient(states, plans[None])
            return np.asarray(ret[0], np.float64), np.asarray(grad[0], np.float64)
        return call
    raise TypeError("refine_plan needs an Engine (plan_gradient) or a DeterministicTrajectoryEvaluator (value_and_gradient), got %s"
                    % type(obj).__name__)


def refine_plan_device(evaluator_or_engine, states, plans, steps, lr, method="adam"):
    """refine_plan with the whole loop on the device (Engine.refine_plans, bbmpc_refine_plans): the
    same rule in float32, the bounds the handle's own.  Takes an Engine, or a DeterministicTrajectoryEvaluator (its rows
    engine, as value_and_gradient).  Returns (plans [B,H,U] in the input's dtype, returns [B] float64); steps = 0 returns
    the input and its return."""
    if method not in ("adam", "sgd"):
        raise ValueError("method must be 'adam' or 'sgd', got %r" % (method,))
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if not (float(lr) > 0.0 and np.isfinite(lr)):
        raise ValueError("lr must be positive and finite")
    plans = np.asarray(plans)
    if plans.ndim != 3:
        raise ValueError("plans must be [B, planning_horizon, dim_U]")
    if hasattr(evaluator_or_engine, "refine_plans"):
        out, ret = evaluator_or_engine.refine_plans(states, plans, steps, lr, method=method, keep_best=True)
    elif hasattr(evaluator_or_engine, "refine_plans_rows"):
        out, ret = evaluator_or_engine.refine_plans_rows(states, plans, steps, lr, method=method)
    else:
        raise TypeError("refine_plan_device needs an Engine (refine_plans) or a DeterministicTrajectoryEvaluator "
                        "(refine_plans_rows), got %s" % type(evaluator_or_engine).__name__)
    return out.astype(plans.dtype), np.asarray(ret, np.float64)


def refine_plan(evaluator_or_engine, states, plans, steps, lr, lo, hi, method="adam"):
    """Projected gradient ascent on the model return of `plans` [B,H,U] from `states` [B,S]: `steps` updates with step size
    `lr` ("adam": Adam with beta 0.9 / 0.999 on the ascent direction; "sgd": plain ascent), each followed by a clip to the
    per-dimension bounds lo, hi [U].  Per row the best plan seen BY THE MODEL RETURN is kept -- the input included -- so the
    result is never worse than what came in, and more steps are never worse than fewer.  Returns (plans [B,H,U] in the
    input's dtype, returns [B] float64).  steps = 0 returns the input and its return."""
    if method not in ("adam", "sgd"):
        raise ValueError("method must be 'adam' or 'sgd', got %r" % (method,))
    steps = int(steps)
    if steps < 0:
        raise ValueError("steps must be >= 0")
    if not (float(lr) > 0.0 and np.isfinite(lr)):
        raise ValueError("lr must be positive and finite")
    call = _backend(evaluator_or_engine)
    plans = np.asarray(plans)
    if plans.ndim != 3:
        raise ValueError("plans must be [B, planning_horizon, dim_U]")
    lo = np.broadcast_to(np.asarray(lo, np.float64), (plans.shape[2],))
    hi = np.broadcast_to(np.asarray(hi, np.float64), (plans.shape[2],))
    x = np.asarray(plans, np.float64).copy()
    best, best_ret = x.copy(), None
    m, v = np.zeros_like(x), np.zeros_like(x)
    for k in range(steps + 1):
        ret, grad = call(states, x.astype(plans.dtype))
        if best_ret is None:
            best_ret = ret.copy()
        else:
            better = ret > best_ret                        # (a NaN return never replaces anything)
            best[better], best_ret[better] = x[better], ret[better]
        if k == steps:
            break
        if method == "adam":
            m = 0.9 * m + 0.1 * grad
            v = 0.999 * v + 0.001 * grad * grad
            step = (m / (1.0 - 0.9 ** (k + 1))) / (np.sqrt(v / (1.0 - 0.999 ** (k + 1))) + 1e-8)
        else:
            step = grad
        x = np.clip(x + float(lr) * np.where(np.isfinite(step), step, 0.0), lo, hi)
        x = x.astype(plans.dtype).astype(np.float64)       # what the backend will see
    return best.astype(plans.dtype), best_ret
