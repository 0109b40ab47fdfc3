"""User-supplied reward / dynamics functions as device code.

The reference accepts any Python (TensorFlow) callable as `reward_function` / `dynamics_function`
(trajectory_evaluators/deterministic.py:13-18).  Here the rollouts run inside GPU kernels, so a user function is HIP
source compiled at run time (hiprtc) and called per row from the engine's step-wise evaluator:

    reward = HipRewardFunction('''
        __device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U) {
            return -(cur[0] * cur[0]) - 0.1f * act[0] * act[0];
        }''')
    dynamics = HipDynamicsFunction('''
        __device__ void bbmpc_user_dynamics(const float* x, float* delta, int S, int U) {   // x = [state | action]
            delta[0] = 0.05f * x[1];  delta[1] = 0.05f * x[2];                              // returns next - state
        }''')
    policy = MPCPolicy(reward_function=reward, dynamics_function=dynamics, true_model=True, ...)

Argument order of the reward is the order of the reference's CALL, `reward_function(current_state, actions,
next_state)` (deterministic.py:65-66).  A user dynamics function is a true model: it returns the state delta and the
handler adds the state back (utils/transforms.py:34).  Both objects are also directly callable with NumPy batches
(they run the same device code through the C ABI), like the built-in plug-ins.

PLAIN CALLABLES (what the reference's users pass) are accepted when they work on PyTorch tensors on the GPU -- the
counterpart of the reference's TensorFlow callables:

    reward = lambda cur, act, nxt: -(cur[:, 0] ** 2) - 0.1 * act[:, 0] ** 2          # torch ops on [B,S] / [B,U] / [B,S]
    dynamics = torch.nn.Sequential(...).cuda()                                       # f(x[B,S+U]) -> [B,S]

The engine then evaluates step by step (SURVEY.md H5's unfused fallback) and calls back once per planning step with
the row batches of its own HBM buffers aliased as torch tensors (TorchRewardFunction / TorchDynamicsFunction below,
bbmpc_set_*_callback in include/bbmpc.h); the torch work is enqueued on the engine's stream, nothing is copied to the
host.  Slower than device code (2 * H + 2 launches plus the framework's per-op overhead) but never on the CPU.  A callable
that cannot take CUDA tensors is refused (NotImplementedError), as before.

RUNTIME PARAMETERS (goals, setpoints, reference trajectories, estimated plant constants) change between control steps
without a recompile.  A function declared with num_params=P defines the parameterised entry point instead
(include/bbmpc.h):

    reward = HipRewardFunction('''
        __device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
                                                  const float* params, int t) {       // params: this agent's P floats
            const float d = nxt[0] - params[0];                                        // t: planning step (0 one-step)
            return -d * d - 0.1f * act[0] * act[0];
        }''', num_params=1)
    reward.set_params([0.5])                        # [P]: every agent; [num_agents_global, P]: one row per agent

Every engine built on the function uploads the parameters before its next computation when they changed (an engine of
a sharded policy takes the rows of its own agents); set_params never compiles."""
import numpy as np

from .. import _lib as L


def check_source(kind, hip_source, dim_s, dim_u):
    """Compile only (no GPU needed); raises BBMPCError with the compiler log on failure."""
    L.check(L.lib.bbmpc_check_user_source(int(kind), hip_source.encode(), int(dim_s), int(dim_u)))


def check_params_source(dim_s, dim_u, reward_source=None, reward_params=0, dynamics_source=None, dynamics_params=0):
    """Compile only (no GPU needed) every program a parameterised reward and / or dynamics takes part in."""
    rew = reward_source.encode() if reward_source is not None else None
    dyn = dynamics_source.encode() if dynamics_source is not None else None
    L.check(L.lib.bbmpc_check_user_params(rew, int(reward_params), dyn, int(dynamics_params), int(dim_s), int(dim_u)))


class _HipFunction:
    num_params = 0
    _params = None                    # float32 [P] (shared) or [num_agents_global, P] (per agent), set_params' copy
    _params_version = 0

    def __init__(self, hip_source):
        if not isinstance(hip_source, str) or not hip_source.strip():
            raise ValueError("hip_source must be a non-empty string of HIP device code")
        self.hip_source = hip_source
        self._engines = {}

    def _init_params(self, num_params):
        if isinstance(num_params, bool) or not isinstance(num_params, (int, np.integer)):
            raise TypeError("num_params must be an int, got %r" % (num_params,))
        if not 0 <= int(num_params) <= L.MAX_USER_PARAMS:
            raise ValueError("num_params must be in [0, %d], got %d" % (L.MAX_USER_PARAMS, num_params))
        self.num_params = int(num_params)

    def set_params(self, values):
        """values [P] (shared by every agent) or [num_agents_global, P] (one row per agent): stored as a float32 copy;
        engines upload it before their next computation."""
        if not self.num_params:
            raise ValueError("set_params: %s was declared without runtime parameters (num_params=0)" % type(self).__name__)
        v = np.array(values, dtype=np.float32, copy=True)
        P = self.num_params
        if not ((v.ndim == 1 and v.shape[0] == P) or (v.ndim == 2 and v.shape[0] >= 1 and v.shape[1] == P)):
            raise ValueError("set_params: expected [%d] or [num_agents_global, %d], got shape %s" % (P, P, v.shape))
        self._params = v
        self._params_version += 1

    def _direct_engine(self, dim_s, dim_u):
        """The engine of a direct NumPy call: shared parameters only."""
        if self._params is not None and self._params.ndim == 2:
            raise ValueError("calling %s directly uses shared parameters, but per-agent ones are set" % type(self).__name__)
        eng = self._engine(dim_s, dim_u)
        sync_user_params(eng)
        return eng

    def _engine(self, dim_s, dim_u, low=None, high=None):
        from ..engine import Engine
        key = (int(dim_s), int(dim_u))
        eng = self._engines.get(key)
        if eng is None:
            lo = np.full(key[1], -1.0, np.float32) if low is None else low
            hi = np.full(key[1], 1.0, np.float32) if high is None else high
            eng = self._make(Engine, key[0], lo, hi)
            self._engines[key] = eng
        return eng


class HipRewardFunction(_HipFunction):
    """reward_function given as HIP source (`bbmpc_user_reward`, or `bbmpc_user_reward_params` with num_params > 0)."""
    _bbmpc_reward_kind = L.REW_USER

    def __init__(self, hip_source, num_params=0):
        super().__init__(hip_source)
        self._init_params(num_params)

    def _make(self, Engine, dim_s, lo, hi):
        # the dynamics kind is irrelevant for evaluate_next_reward; a user-dynamics handle needs no weights
        eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, lo, hi, dim_s=dim_s, num_agents=1, planning_horizon=1)
        eng.set_reward_source(self.hip_source, self.num_params)
        attach_params(eng, L.USER_KIND_REWARD, self)
        return eng

    def __call__(self, current_state, actions, next_state):
        cur, act, nxt = (np.asarray(v, np.float32) for v in (current_state, actions, next_state))
        return self._direct_engine(cur.shape[1], act.shape[1]).evaluate_next_reward(cur, nxt, act)


class HipDynamicsFunction(_HipFunction):
    """dynamics_function given as HIP source (`bbmpc_user_dynamics`, or `bbmpc_user_dynamics_params` with
    num_params > 0); f(x[B,S+U], train) -> delta[B,S]."""
    _bbmpc_dynamics_kind = L.DYN_USER

    def __init__(self, hip_source, dim_s=None, dim_u=None, num_params=0):
        super().__init__(hip_source)
        self._dims = (dim_s, dim_u)
        self._init_params(num_params)

    def _make(self, Engine, dim_s, lo, hi):
        eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, lo, hi, dim_s=dim_s, num_agents=1, planning_horizon=1)
        eng.set_dynamics_source(self.hip_source, self.num_params)
        attach_params(eng, L.USER_KIND_DYNAMICS, self)
        return eng

    def __call__(self, x, train=False):
        x = np.asarray(x, np.float32)
        dim_s, dim_u = self._dims
        if dim_s is None or dim_u is None:
            raise ValueError("calling a HipDynamicsFunction directly needs dim_s / dim_u (constructor) to split x")
        s, a = x[:, :dim_s], x[:, dim_s:dim_s + dim_u]
        return self._direct_engine(dim_s, dim_u).predict_next_state(s, a) - s


class HipInverseTargetTransform(_HipFunction):
    """inverse_transform_targets_func given as HIP source (`bbmpc_user_inverse_transform_targets(cur, dev, next, S)`):
    next = g(state, dev), where dev is the de-normalised model output (the raw output of a true / un-normalised model) --
    the reference's process_output order (system_dynamics_handler.py:128-161).  Inlined into the learned-model rollout
    kernel and the HIP-source true model's kernels; callable on NumPy batches: (states[B,S], dev[B,S]) -> next[B,S]."""
    _bbmpc_transform_kind = L.USER_KIND_INVERSE_TRANSFORM

    def _make(self, Engine, dim_s, lo, hi):
        eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, lo, hi, dim_s=dim_s, num_agents=1, planning_horizon=1)
        eng.set_inverse_transform_source(self.hip_source)
        return eng

    def __call__(self, states, dev):
        s, d = np.asarray(states, np.float32), np.asarray(dev, np.float32)
        return self._engine(s.shape[1], 1).transform_rows(L.USER_KIND_INVERSE_TRANSFORM, s, d)


class HipTargetTransform(_HipFunction):
    """transform_targets_func given as HIP source (`bbmpc_user_transform_targets(cur, next, target, S)`): what a learned
    model is trained to predict (system_dynamics_handler.py:314).  Callable on NumPy batches:
    (states[T,S], next_states[T,S]) -> targets[T,S], on the GPU."""
    _bbmpc_transform_kind = L.USER_KIND_TRANSFORM

    def _make(self, Engine, dim_s, lo, hi):
        eng = Engine(L.OPT_NONE, L.DYN_USER, L.REW_USER, lo, hi, dim_s=dim_s, num_agents=1, planning_horizon=1)
        eng.set_transform_source(self.hip_source)
        return eng

    def __call__(self, states, next_states):
        s, n = np.asarray(states, np.float32), np.asarray(next_states, np.float32)
        return self._engine(s.shape[1], 1).transform_rows(L.USER_KIND_TRANSFORM, s, n)


def attach_params(engine, kind, fn):
    """Register a parameterised function with the engine it was just set on (the handle has no parameters yet)."""
    engine._params_uploaded.pop(kind, None)
    if fn.num_params:
        engine._param_fns[kind] = fn
    else:
        engine._param_fns.pop(kind, None)


def sync_user_params(engine):
    """Upload the parameters of the engine's parameterised functions whose copy on the engine is behind: a shared row,
    or the rows [agent_offset, agent_offset + num_agents) of per-agent ones.  Never set: left to the engine to refuse."""
    for kind, fn in engine._param_fns.items():
        p = fn._params
        if p is None or engine._params_uploaded.get(kind) == fn._params_version:
            continue
        if p.ndim == 2:
            if p.shape[0] != engine.cfg.num_agents_global:
                raise ValueError("%s: per-agent parameters have %d rows, the engine plans for %d agents"
                                 % (type(fn).__name__, p.shape[0], engine.cfg.num_agents_global))
            p = p[engine.cfg.agent_offset:engine.cfg.agent_offset + engine.A]
        engine.set_user_params(kind, p)
        engine._params_uploaded[kind] = fn._params_version


def check_transform_rollout(hip_source, dim_s, dim_u, reward_kind=L.REW_CHEETAH, reward_source=None):
    """Compile only (no GPU needed) the learned-model rollout with this inverse target transform (and reward) inlined."""
    rew = reward_source.encode() if reward_source is not None else None
    L.check(L.lib.bbmpc_check_xform_rollout(int(reward_kind), hip_source.encode(), rew, int(dim_s), int(dim_u)))


# ---- plain callables on torch CUDA tensors --------------------------------------------------------------------------------
class _DeviceBlock:
    """A float32 block of the engine's device memory as an object torch.as_tensor aliases without a copy."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(int(v) for v in shape), "typestr": "<f4", "data": (int(ptr), False),
                                         "version": 2}


class _TorchCallback:
    """Common half of the two adapters: the ctypes callback, the torch stream that IS the engine's stream, error parking."""

    def __init__(self, fn):
        if not callable(fn):
            raise TypeError("expected a callable, got %r" % (fn,))
        self.fn = fn
        self._streams = {}
        self._engines = {}

    def _alias(self, torch, ptr, shape, device):
        return torch.as_tensor(_DeviceBlock(ptr, shape), device=device)

    def _stream(self, torch, ptr, device):
        st = self._streams.get(ptr)
        if st is None:
            st = self._streams[ptr] = torch.cuda.ExternalStream(int(ptr), device=device) if ptr else torch.cuda.default_stream(device)
        return st

    def _guard(self, body):
        def cb(user, d_cur, d_act, d_next, batch, d_out, stream):
            try:
                body(d_cur, d_act, d_next, int(batch), d_out, stream or 0)
                return 0
            except BaseException as ex:                   # noqa: BLE001 -- nothing may unwind through the C frames
                L.park_callback_error(ex)
                return 1
        return L.ROWS_CALLBACK(cb)

    @staticmethod
    def _result(torch, r, shape, what):
        if not torch.is_tensor(r) or not r.is_cuda:
            raise TypeError("%s must return a torch tensor on the GPU, got %s" % (what, type(r).__name__))
        return r.to(torch.float32).reshape(shape)


class TorchRewardFunction(_TorchCallback):
    """reward_function(current_state[B,S], actions[B,U], next_state[B,S]) -> [B] on torch CUDA tensors
    (the argument order of the reference's call, deterministic.py:65-66)."""
    _bbmpc_reward_kind = L.REW_USER

    def make_callback(self, dim_s, dim_u, device):
        import torch
        dev = torch.device("cuda", int(device))

        def body(d_cur, d_act, d_next, batch, d_out, stream):
            with torch.cuda.stream(self._stream(torch, stream, dev)):
                cur = self._alias(torch, d_cur, (batch, dim_s), dev)
                act = self._alias(torch, d_act, (batch, dim_u), dev)
                nxt = self._alias(torch, d_next, (batch, dim_s), dev)
                out = self._alias(torch, d_out, (batch,), dev)
                out.copy_(self._result(torch, self.fn(cur, act, nxt), (batch,), "reward_function"))
        return self._guard(body)

    def probe(self, dim_s, dim_u, device):
        import torch
        dev = torch.device("cuda", int(device))
        z = lambda *shape: torch.zeros(shape, device=dev)
        self._result(torch, self.fn(z(2, dim_s), z(2, dim_u), z(2, dim_s)), (2,), "reward_function")

    def __call__(self, current_state, actions, next_state):
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        t = lambda v: torch.as_tensor(np.asarray(v, np.float32), device=dev)
        return self.fn(t(current_state), t(actions), t(next_state)).to(torch.float32).cpu().numpy()


def _takes_train_argument(fn):
    """Does dynamics_function accept a second positional argument (the reference's `train`, deterministic.py:99-100)?
    Decided ONCE from the signature: calling fn(x, False) and retrying fn(x) on TypeError would hide a TypeError raised
    inside the function itself."""
    import inspect
    try:
        params = list(inspect.signature(fn).parameters.values())
    except (TypeError, ValueError):
        return True                                       # no introspectable signature: the reference's call form
    if any(p.kind == p.VAR_POSITIONAL for p in params):
        return True
    positional = [p for p in params if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
    return len(positional) >= 2


def call_torch_dynamics(fn, x):
    """dynamics_function(x, train=False) (deterministic.py:99-100); a torch.nn.Module, or a callable of one argument,
    takes x alone."""
    import torch
    if isinstance(fn, torch.nn.Module):
        return fn(x)
    takes = getattr(fn, "_bbmpc_takes_train", None)
    if takes is None:
        takes = _takes_train_argument(fn)
        try:
            fn._bbmpc_takes_train = takes
        except (AttributeError, TypeError):
            pass
    return fn(x, False) if takes else fn(x)


class TorchDynamicsFunction(_TorchCallback):
    """dynamics_function(x[B,S+U], train) -> raw[B,S] on torch CUDA tensors; the handler's process_input / process_output
    (system_dynamics_handler.py:97-161, utils/transforms.py:20-34) run around it in torch, on the same stream."""
    _bbmpc_dynamics_kind = L.DYN_USER

    def make_callback(self, handler, device):
        import torch
        dev = torch.device("cuda", int(device))
        dim_s, dim_u = handler._dim_S, handler._dim_U
        step = self.stepper(handler, dev)

        def body(d_cur, d_act, d_next, batch, d_out, stream):
            with torch.cuda.stream(self._stream(torch, stream, dev)):
                cur = self._alias(torch, d_cur, (batch, dim_s), dev)
                act = self._alias(torch, d_act, (batch, dim_u), dev)
                out = self._alias(torch, d_out, (batch, dim_s), dev)
                out.copy_(step(cur, act))
        return self._guard(body)

    def stepper(self, handler, dev):
        """(states, actions) -> absolute next states, op for op what the handler does around the model."""
        import torch
        dim_s = handler._dim_S
        stats = handler.normalization_stats()
        inverse = getattr(handler, "_inverse_transform_targets_func", None)
        if stats is not None:
            ms, ss, ma, sa, mt, st_ = (torch.as_tensor(v, device=dev) for v in stats)
            ss, sa, st_ = ss + 1e-7, sa + 1e-7, st_ + 1e-7

        def step(cur, act):
            if stats is None:
                x = torch.cat([cur, act], dim=1)                                   # :104-108
            else:
                x = torch.cat([(cur - ms) / ss, (act - ma) / sa], dim=1)           # :109-125
            raw = self._result(torch, call_torch_dynamics(self.fn, x), (cur.shape[0], dim_s), "dynamics_function")
            if stats is not None:
                raw = mt + raw * st_                                                # :150-156
            return inverse(cur, raw) if inverse is not None else raw + cur          # transforms.py:34
        return step

    def probe(self, handler, device):
        import torch
        dev = torch.device("cuda", int(device))
        step = self.stepper(handler, dev)
        out = step(torch.zeros((2, handler._dim_S), device=dev), torch.zeros((2, handler._dim_U), device=dev))
        self._result(torch, out, (2, handler._dim_S), "dynamics_function")

    def __call__(self, x, train=False):
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        return call_torch_dynamics(self.fn, torch.as_tensor(np.asarray(x, np.float32), device=dev)).to(torch.float32).cpu().numpy()


_torch_plugins = {}                                        # fallback for callables that take no attributes (builtins, slots)


def torch_plugin(fn, cls):
    """The adapter of a plain callable, one per callable object: kept on the callable itself when it takes attributes
    (functions, lambdas, torch modules), so that it lives exactly as long as the callable does."""
    attr = "_bbmpc_" + cls.__name__
    p = getattr(fn, attr, None) or _torch_plugins.get((id(fn), cls))
    if isinstance(p, cls) and p.fn is fn:
        return p
    p = cls(fn)
    try:
        object.__setattr__(fn, attr, p)
    except (AttributeError, TypeError):
        _torch_plugins[(id(fn), cls)] = p                 # (holds fn through p.fn: the id cannot be recycled)
    return p


def gpu_for_callables():
    """The device index torch callables run on, or None when there is no GPU (or no torch) to run them."""
    try:
        import torch
        if torch.cuda.is_available():
            return torch.cuda.current_device()
    except Exception:                                     # noqa: BLE001
        pass
    return None
