"""Plan refinement on the device (bbmpc_refine_plans, bbmpc_set_grad_refine): the NumPy statement of one
update and of a whole refinement, shared by tests/test_plan_refine_cpu.py and tests/test_gpu_plan_refine.py.  Test
infrastructure only.

One update (csrc/kernels_plan_refine.hpp's order, every operation in `dt`), k the 1-based step number:
    Adam:  m = 0.9 m + 0.1 g;  v = 0.999 v + (0.001 g) g
           step = (m / c1) / (sqrt(v / c2) + 1e-8),  c1 = 1 - 0.9^k, c2 = 1 - 0.999^k
    SGD:   step = g
    step = step where finite, else 0
    x = clip(x + lr * step, lo[u], hi[u])
np.float64 is the statement (the arithmetic of utils.plan_refinement.refine_plan); np.float32 restates the kernel: the powers
0.9^k and 0.999^k are k float32 products, as the host forms them for the kernel.

A refinement: steps + 1 gradient calls with keep-best (the input included, `ret > best_ret`, so a NaN return never replaces
anything), or `steps` calls and the last iterate without.  After every update x is rounded to the plans' dtype, which is what
the next gradient call sees (refine_plan does the same)."""
import numpy as np

F = np.float32


def bias_correction(k, dt):
    dt = np.dtype(dt).type
    if dt is np.float32:
        p1, p2 = F(1), F(1)
        for _ in range(k):
            p1, p2 = F(p1 * F(0.9)), F(p2 * F(0.999))
        return F(1) - p1, F(1) - p2
    return dt(1.0 - 0.9 ** k), dt(1.0 - 0.999 ** k)


def update(x, g, m, v, k, lr, lo, hi, method, dt=np.float64):
    """one step -> (x, m, v), all in dt; x [B, H, U], lo / hi [U]"""
    dt = np.dtype(dt).type
    x, g, m, v = (np.asarray(a, dt) for a in (x, g, m, v))
    lo, hi = np.asarray(lo, dt), np.asarray(hi, dt)
    with np.errstate(all="ignore"):
        if method == "adam":
            m = dt(0.9) * m + dt(0.1) * g
            v = dt(0.999) * v + (dt(0.001) * g) * g
            c1, c2 = bias_correction(k, dt)
            step = (m / c1) / (np.sqrt(v / c2) + dt(1e-8))
        elif method == "sgd":
            step = g
        else:
            raise ValueError(method)
        step = np.where(np.isfinite(step), step, dt(0))
        x = np.minimum(np.maximum(x + dt(lr) * step, lo), hi)
    assert x.dtype == dt and m.dtype == dt and v.dtype == dt
    return x, m, v


def keep_best(x, ret, best, best_ret):
    """(best, best_ret) after the plans x scored ret; best_ret None: the first call of a refinement"""
    if best_ret is None:
        return x.copy(), ret.copy()
    better = ret > best_ret
    best, best_ret = best.copy(), best_ret.copy()
    best[better], best_ret[better] = x[better], ret[better]
    return best, best_ret


def refine(value_and_grad, states, plans, steps, lr, lo, hi, method, keep=True, dt=np.float64):
    """value_and_grad(states, plans in the plans' dtype) -> (returns [B], grad [B, H, U]).  -> (plans in dt, returns in dt)"""
    dt = np.dtype(dt).type
    plans = np.asarray(plans)
    x = plans.astype(dt)
    m, v = np.zeros_like(x), np.zeros_like(x)
    best, best_ret = None, None
    for k in range(steps + 1):
        if k == steps and not keep:
            break
        ret, g = value_and_grad(states, x.astype(plans.dtype))
        if keep:
            best, best_ret = keep_best(x, np.asarray(ret, dt), best, best_ret)
        if k == steps:
            break
        x, m, v = update(x, g, m, v, k + 1, lr, lo, hi, method, dt)
        x = x.astype(plans.dtype).astype(dt)
    if keep:
        return best, best_ret
    return x, np.asarray(value_and_grad(states, x.astype(plans.dtype))[0], dt)
