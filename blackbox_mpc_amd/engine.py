"""Thin object wrapper over the C ABI handle (include/bbmpc.h).  NumPy in, NumPy
out; device-pointer variants take integer addresses (e.g. torch `data_ptr()`)."""
import ctypes
import os

import numpy as np

from . import _lib as L


class Engine:
    risk = (L.RISK_MEAN_STD, 0)        # (kind, tail_count) of set_particle_risk: a new handle scores mean - kappa * std
    _lib = L.lib                       # the library whose bbmpc_optimize / bbmpc_optimize_gather the hot path calls
    _fastcall_on = True                # BBMPC_FASTCALL=0 at creation: the hot path stays on ctypes (A/B runs, parity tests)
    _fast = None                       # the _fastcall object bound to this handle; None: not bound yet, False: ctypes path

    def __init__(self, optimizer, dynamics, reward, action_low, action_high, dim_s, num_agents,
                 planning_horizon, population_size=0, max_iterations=0, num_elite=0, seed=0, quirks=0,
                 agent_offset=0, num_agents_global=None, device=-1, alpha=0.25, lamda=1.0,
                 pso_c1=0.3, pso_c2=0.5, pso_w=0.2, pso_v0_fraction=0.01,
                 spsa_alpha=0.602, spsa_gamma=0.101, spsa_a=0.01, spsa_c=0.3,
                 cma_alpha_cov=2.0, cma_h_sigma=1.0, population_offset=0, population_global=0):
        self._h = ctypes.c_void_p()
        self._fastcall_on = os.environ.get("BBMPC_FASTCALL", "1") != "0"
        self._lo = L.f32c(np.asarray(action_low).reshape(-1))
        self._hi = L.f32c(np.asarray(action_high).reshape(-1))
        if self._lo.shape != self._hi.shape:
            raise ValueError("action_low/action_high shapes differ")
        c = L.Config()
        c.abi_version = L.ABI_VERSION
        c.optimizer, c.dynamics, c.reward = int(optimizer), int(dynamics), int(reward)
        c.population_size, c.num_agents = int(population_size), int(num_agents)
        c.planning_horizon, c.dim_u, c.dim_s = int(planning_horizon), int(self._lo.shape[0]), int(dim_s)
        c.max_iterations = int(max_iterations or 0)
        c.num_elite = int(num_elite)
        c.agent_offset = int(agent_offset)
        c.num_agents_global = int(num_agents_global if num_agents_global is not None else num_agents)
        c.device = int(device)
        c.quirks = int(quirks)
        c.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        c.alpha, c.lamda = float(alpha), float(lamda)
        c.pso_c1, c.pso_c2, c.pso_w, c.pso_v0_fraction = float(pso_c1), float(pso_c2), float(pso_w), float(pso_v0_fraction)
        c.spsa_alpha, c.spsa_gamma, c.spsa_a, c.spsa_c = float(spsa_alpha), float(spsa_gamma), float(spsa_a), float(spsa_c)
        c.cma_alpha_cov, c.cma_h_sigma = float(cma_alpha_cov), float(cma_h_sigma)
        c.population_offset, c.population_global = int(population_offset), int(population_global or 0)
        c.action_low = self._lo.ctypes.data_as(L.c_float_p)
        c.action_high = self._hi.ctypes.data_as(L.c_float_p)
        self.cfg = c
        self.N, self.A, self.H = c.population_size, c.num_agents, c.planning_horizon
        self.U, self.S = c.dim_u, c.dim_s
        self.iters = 1 if optimizer == L.OPT_RANDOM_SEARCH else c.max_iterations
        self.k = c.num_elite
        L.check(L.lib.bbmpc_create(ctypes.byref(c), ctypes.byref(self._h)))
        dev = ctypes.c_int32(-1)
        L.check(L.lib.bbmpc_handle_device(self._h, ctypes.byref(dev)))             # where the handle lives, fixed at creation: the
        self._device = int(dev.value)                                               # library's answer, not a guess from torch's state
        self._param_fns, self._params_uploaded = {}, {}     # parameterised user functions: kind -> function / uploaded version

    @property
    def device(self):
        """The GPU this handle lives on: bbmpc_config.device, or (-1) the process's current device AT CREATION -- the
        torch callbacks alias the engine's HBM pointers and stream on this device whatever is current later."""
        return self._device

    # -- lifecycle -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            L.lib.bbmpc_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._fast = None                  # (it holds the handle's address)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_ptr):
        """Launch on the given hipStream_t handle; 0 / None = the handle's own stream (include/bbmpc.h)."""
        L.check(L.lib.bbmpc_set_stream(self._h, ctypes.c_void_p(stream_ptr or 0)))

    def set_torch_stream(self, stream):
        """Launch on a torch.cuda.Stream so that torch work on that stream (events, collectives, copies) is ordered
        with the engine's kernels.  PyTorch's default stream has the NULL handle, which bbmpc_set_stream reads as
        "the handle's own stream": it goes through bbmpc_set_stream_default."""
        ptr = int(stream.cuda_stream)
        if ptr != 0:
            self.set_stream(ptr)
        else:
            L.check(L.lib.bbmpc_set_stream_default(self._h))

    def set_mlp(self, weights, biases, activations, stats=None):
        n = len(weights)
        ws = [L.f32c(w) for w in weights]
        bs = [L.f32c(b) for b in biases]
        dims = [ws[0].shape[0]] + [w.shape[1] for w in ws]
        for i, (w, b) in enumerate(zip(ws, bs)):
            if w.ndim != 2 or w.shape[0] != dims[i] or b.shape != (w.shape[1],):
                raise ValueError("layer %d: kernel must be [in,out] and bias [out]" % i)
        dims_a = (ctypes.c_int32 * (n + 1))(*dims)
        acts_a = (ctypes.c_int32 * n)(*[int(a) for a in activations])
        wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        if stats is not None:
            st = [L.f32c(np.asarray(s).reshape(-1)) for s in stats]
            sp = (ctypes.c_void_p * 6)(*[s.ctypes.data for s in st])
            L.check(L.lib.bbmpc_set_mlp(self._h, n, dims_a, acts_a, wp, bp, 1, sp))
        else:
            L.check(L.lib.bbmpc_set_mlp(self._h, n, dims_a, acts_a, wp, bp, 0, None))
        self._mlp_last_hidden = dims[-2]                 # rows of a log-variance head's kernel (set_mlp_logvar_head)

    def set_reward_mlp(self, weights, biases, activations, input_mask=7, stats=None):
        """Learned reward model of a DYN_MLP + REW_MLP handle (bbmpc_set_reward_mlp): Dense kernels [in, out] / biases [out]
        ending in one output, any ACT_* code per layer; input_mask bit 0 = s_t, 1 = a_t, 2 = s_{t+1} (concatenated in that
        order); stats = (mean_in [D], std_in [D], mean_r, std_r) or None."""
        n = len(weights)
        ws = [L.f32c(w) for w in weights]
        bs = [L.f32c(np.asarray(b).reshape(-1)) for b in biases]
        dims = [ws[0].shape[0]] + [w.shape[1] for w in ws]
        for i, (w, b) in enumerate(zip(ws, bs)):
            if w.ndim != 2 or w.shape[0] != dims[i] or b.shape != (w.shape[1],):
                raise ValueError("layer %d: kernel must be [in,out] and bias [out]" % i)
        dims_a = (ctypes.c_int32 * (n + 1))(*dims)
        acts_a = (ctypes.c_int32 * n)(*[int(a) for a in activations])
        wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        if stats is not None:
            st = [L.f32c(np.asarray(s).reshape(-1)) for s in stats]
            sp = (ctypes.c_void_p * 4)(*[s.ctypes.data for s in st])
            L.check(L.lib.bbmpc_set_reward_mlp(self._h, n, dims_a, acts_a, wp, bp, int(input_mask), 1, sp))
        else:
            L.check(L.lib.bbmpc_set_reward_mlp(self._h, n, dims_a, acts_a, wp, bp, int(input_mask), 0, None))

    def set_terminal_value_mlp(self, weights, biases, activations, stats=None, terminal_weight=1.0):
        """Learned terminal value of a DYN_MLP handle (bbmpc_set_terminal_value_mlp): Dense kernels [in, out] / biases [out]
        from dim_S inputs to one output, any ACT_* code per layer; stats = (mean_in [S], std_in [S], mean_v, std_v) or
        None.  Rollout scores become R + terminal_weight * V(s_H).  weights = None (or an empty list) removes the network."""
        if not weights:
            L.check(L.lib.bbmpc_set_terminal_value_mlp(self._h, 0, None, None, None, None, 0, None, 0.0))
            return
        n = len(weights)
        ws = [L.f32c(w) for w in weights]
        bs = [L.f32c(np.asarray(b).reshape(-1)) for b in biases]
        dims = [ws[0].shape[0]] + [w.shape[1] for w in ws]
        for i, (w, b) in enumerate(zip(ws, bs)):
            if w.ndim != 2 or w.shape[0] != dims[i] or b.shape != (w.shape[1],):
                raise ValueError("layer %d: kernel must be [in,out] and bias [out]" % i)
        dims_a = (ctypes.c_int32 * (n + 1))(*dims)
        acts_a = (ctypes.c_int32 * n)(*[int(a) for a in activations])
        wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        sp = None
        if stats is not None:
            st = [L.f32c(np.asarray(s).reshape(-1)) for s in stats]
            if st[0].shape != (dims[0],) or st[1].shape != (dims[0],) or st[2].shape != (1,) or st[3].shape != (1,):
                raise ValueError("stats must be (mean_in [%d], std_in [%d], mean_v [1], std_v [1])" % (dims[0], dims[0]))
            sp = (ctypes.c_void_p * 4)(*[s.ctypes.data for s in st])
        L.check(L.lib.bbmpc_set_terminal_value_mlp(self._h, n, dims_a, acts_a, wp, bp, 1 if stats is not None else 0, sp,
                                                   float(terminal_weight)))

    def evaluate_terminal_value(self, states):
        """V on rows (bbmpc_evaluate_terminal_value): states [B, S] -> [B], without the weight and without a NaN rule."""
        states = L.f32c(states)
        b = states.shape[0] if states.ndim == 2 else -1
        if states.shape != (b, self.S):                  # the C side copies b * S floats from this buffer
            raise ValueError("states [B,%d] expected, got %s" % (self.S, states.shape))
        out = np.empty((b,), np.float32)
        if b:
            L.check(L.lib.bbmpc_evaluate_terminal_value(self._h, L.ptr(states), b, L.ptr(out)))
        return out

    def evaluate_terminal_value_dev(self, d_states, batch, d_values):
        L.check(L.lib.bbmpc_evaluate_terminal_value_dev(self._h, ctypes.c_void_p(d_states), int(batch), ctypes.c_void_p(d_values)))

    def set_return_shaping(self, discount=1.0, state_low=None, state_high=None, terminal_reward=0.0):
        """Discounted, termination-aware returns of a DYN_MLP handle (bbmpc_set_return_shaping): candidates score
        sum_t discount^t r_t up to the first state outside [state_low, state_high] (each None or [dim_S], -inf / +inf =
        unbounded), plus discount^T * terminal_reward there, or plus discount^H * w * V(s_H) when they never leave the box
        and a value network is installed.  discount = 1 with both bounds None switches shaping off."""
        bounds = []
        for b in (state_low, state_high):
            if b is not None:
                b = L.f32c(np.asarray(b, np.float32).reshape(-1))
                if b.shape != (self.S,):         # the C side reads dim_S floats from this buffer
                    raise ValueError("a state bound must be [%d], got %s" % (self.S, b.shape))
            bounds.append(b)
        L.check(L.lib.bbmpc_set_return_shaping(self._h, float(discount), L.ptr(bounds[0]), L.ptr(bounds[1]), float(terminal_reward)))

    def termination_steps(self, n_pop=None):
        """T of the most recent rollout (bbmpc_get_termination_steps): int32 [n_pop, A] in evaluate's layout, the first
        terminal step in 1 .. H, 0 = the candidate never left the box.  n_pop: the candidates of that rollout -- by
        default what the handle says it rolled out (bbmpc_get_state "shaping_n_pop")."""
        n = int(n_pop if n_pop is not None else self.get_state("shaping_n_pop", (1,))[0])
        out = np.empty((self.A, max(1, n)), np.int32)
        L.check(L.lib.bbmpc_get_termination_steps(self._h, L.ptr(out), int(out.size)))
        return np.ascontiguousarray(out.T)

    def set_mlp_ensemble(self, members):
        """Model ensemble for the particle rollouts (bbmpc_set_mlp_ensemble): `members` is a list of (weights, biases)
        pairs or of objects with `.weights` / `.biases`, each of the shape of the model set_mlp installed; particle p
        follows member p % len(members).  An empty list / None removes the ensemble."""
        members = list(members or [])
        if not members:
            L.check(L.lib.bbmpc_set_mlp_ensemble(self._h, 0, None, None))
            return
        pairs = [(m.weights, m.biases) if hasattr(m, "weights") else m for m in members]
        ws = [[L.f32c(w) for w in p[0]] for p in pairs]
        bs = [[L.f32c(b) for b in p[1]] for p in pairs]
        n = len(ws[0])
        for e, (w_e, b_e) in enumerate(zip(ws, bs)):
            if len(w_e) != n or len(b_e) != n:
                raise ValueError("member %d: %d layers expected" % (e, n))
            for i, (w, b) in enumerate(zip(w_e, b_e)):
                if w.shape != ws[0][i].shape or b.shape != (w.shape[1],):
                    raise ValueError("member %d, layer %d: kernel %s / bias %s do not match member 0's %s"
                                     % (e, i, w.shape, b.shape, ws[0][i].shape))
        wp = (ctypes.c_void_p * (len(ws) * n))(*[w.ctypes.data for w_e in ws for w in w_e])
        bp = (ctypes.c_void_p * (len(bs) * n))(*[b.ctypes.data for b_e in bs for b in b_e])
        L.check(L.lib.bbmpc_set_mlp_ensemble(self._h, len(ws), wp, bp))

    def set_mlp_logvar_head(self, heads, min_logvar=None, max_logvar=None):
        """Log-variance heads for the particle rollouts (bbmpc_set_mlp_logvar_head): `heads` is a list of (W_v, b_v) pairs
        or of objects with `.logvar_weights` / `.logvar_bias`, one per model the handle rolls -- one per ensemble member,
        else one; min_logvar / max_logvar are scalars or [dim_S].  Call it after set_mlp / set_mlp_ensemble.  An empty
        list / None removes the heads."""
        heads = list(heads or [])
        if not heads:
            L.check(L.lib.bbmpc_set_mlp_logvar_head(self._h, 0, None, None, None, None))
            return
        pairs = [(m.logvar_weights, m.logvar_bias) if hasattr(m, "logvar_weights") else m for m in heads]
        ws = [L.f32c(p[0]) for p in pairs]
        bs = [L.f32c(p[1]) for p in pairs]
        for e, (w, b) in enumerate(zip(ws, bs)):
            hid = getattr(self, "_mlp_last_hidden", w.shape[0] if w.ndim == 2 else -1)    # (no model yet: the ABI refuses)
            if w.shape != (hid, self.S) or b.shape != (self.S,):
                raise ValueError("head %d: kernel %s / bias %s, expected [%d, %d] / [%d]" % (e, w.shape, b.shape, hid, self.S, self.S))
        if min_logvar is None or max_logvar is None:
            raise ValueError("min_logvar and max_logvar are required with heads")
        lo = L.f32c(np.broadcast_to(np.asarray(min_logvar, np.float32), (self.S,)))
        hi = L.f32c(np.broadcast_to(np.asarray(max_logvar, np.float32), (self.S,)))
        wp = (ctypes.c_void_p * len(ws))(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * len(bs))(*[b.ctypes.data for b in bs])
        L.check(L.lib.bbmpc_set_mlp_logvar_head(self._h, len(ws), wp, bp, lo.ctypes.data, hi.ctypes.data))

    def set_reward_source(self, hip_source, num_params=0):
        """HIP source defining `__device__ float bbmpc_user_reward(cur, act, nxt, S, U)`, or with num_params > 0
        `bbmpc_user_reward_params(cur, act, nxt, S, U, params, t)` (include/bbmpc.h)."""
        if num_params:
            L.check(L.lib.bbmpc_set_reward_source_params(self._h, hip_source.encode(), int(num_params)))
        else:
            L.check(L.lib.bbmpc_set_reward_source(self._h, hip_source.encode()))

    def set_dynamics_source(self, hip_source, num_params=0):
        """HIP source defining `__device__ void bbmpc_user_dynamics(x, delta, S, U)`, or with num_params > 0
        `bbmpc_user_dynamics_params(x, delta, S, U, params, t)` (include/bbmpc.h)."""
        if num_params:
            L.check(L.lib.bbmpc_set_dynamics_source_params(self._h, hip_source.encode(), int(num_params)))
        else:
            L.check(L.lib.bbmpc_set_dynamics_source(self._h, hip_source.encode()))

    def set_user_params(self, kind, values):
        """Upload runtime parameters (kind USER_KIND_REWARD / USER_KIND_DYNAMICS): [P] shared or [num_agents, P] (local
        agents).  Never compiles."""
        v = L.f32c(values).reshape(-1)
        L.check(L.lib.bbmpc_set_user_params(self._h, int(kind), L.ptr(v), int(v.size)))

    def compile_count(self):
        """hiprtc compilations this handle has run (bbmpc_compile_stats)."""
        n = ctypes.c_int64(0)
        L.check(L.lib.bbmpc_compile_stats(self._h, ctypes.byref(n)))
        return int(n.value)

    def set_inverse_transform_source(self, hip_source):
        """HIP source defining `__device__ void bbmpc_user_inverse_transform_targets(cur, dev, next, S)`, or None to clear
        (include/bbmpc.h): replaces next = dev + state on a learned-model / user-dynamics handle."""
        L.check(L.lib.bbmpc_set_inverse_transform_source(self._h, hip_source.encode() if hip_source else None))

    def set_transform_source(self, hip_source):
        """HIP source defining `__device__ void bbmpc_user_transform_targets(cur, next, target, S)`, or None to clear."""
        L.check(L.lib.bbmpc_set_transform_source(self._h, hip_source.encode() if hip_source else None))

    def transform_rows(self, kind, states, other):
        """kind USER_KIND_INVERSE_TRANSFORM: (states, dev) -> next; USER_KIND_TRANSFORM: (states, next) -> targets."""
        states, other = L.f32c(states), L.f32c(other)
        b = states.shape[0] if states.ndim == 2 else -1
        if states.shape != (b, self.S) or other.shape != (b, self.S):
            raise ValueError("two [B,%d] arrays expected, got %s, %s" % (self.S, states.shape, other.shape))
        out = np.empty((b, self.S), np.float32)
        if b:
            L.check(L.lib.bbmpc_transform_rows(self._h, int(kind), L.ptr(states), L.ptr(other), b, L.ptr(out)))
        return out

    def set_reward_callback(self, fn):
        """fn(d_cur, d_actions, d_next, batch, d_out, hip_stream) -> status, all device pointers (include/bbmpc.h
        bbmpc_rows_callback); `fn` is an _lib.ROWS_CALLBACK the caller keeps alive; None clears it."""
        self._rew_cb = fn
        L.check(L.lib.bbmpc_set_reward_callback(self._h, fn if fn is not None else L.ROWS_CALLBACK(), None))

    def set_dynamics_callback(self, fn):
        self._dyn_cb = fn
        L.check(L.lib.bbmpc_set_dynamics_callback(self._h, fn if fn is not None else L.ROWS_CALLBACK(), None))

    def mlp_forward(self, x):
        """DeterministicMLP.__call__ on the device: raw Dense stack on processed inputs [B, S+U] -> [B, S]."""
        x = L.f32c(x)
        if x.ndim != 2 or x.shape[1] != self.S + self.U:
            raise ValueError("x must be [B, dim_S + dim_U] = [B, %d], got %s" % (self.S + self.U, x.shape))
        out = np.empty((x.shape[0], self.S), np.float32)
        if x.shape[0]:
            L.check(L.lib.bbmpc_mlp_forward(self._h, L.ptr(x), x.shape[0], L.ptr(out)))
        return out

    def _process(self, fn, first, second, width_second, width_out, stats):
        first, second = L.f32c(first), L.f32c(second)
        b = first.shape[0] if first.ndim == 2 else -1
        if first.shape != (b, self.S) or second.shape != (b, width_second):
            raise ValueError("expected [B,%d] and [B,%d], got %s and %s" % (self.S, width_second, first.shape, second.shape))
        out = np.empty((b, width_out), np.float32)
        if b:
            if stats is not None:
                st = [L.f32c(np.asarray(v).reshape(-1)) for v in stats]
                sp = (ctypes.c_void_p * 6)(*[v.ctypes.data for v in st])
            else:
                sp = None
            L.check(fn(self._h, L.ptr(first), L.ptr(second), b, sp, L.ptr(out)))
        return out

    def process_input(self, states, actions, stats=None):
        return self._process(L.lib.bbmpc_process_input, states, actions, self.U, self.S + self.U, stats)

    def process_output(self, states, raw_output, stats=None):
        return self._process(L.lib.bbmpc_process_output, states, raw_output, self.S, self.S, stats)

    def reset(self):
        L.check(L.lib.bbmpc_reset(self._h))

    def synchronize(self):
        L.check(L.lib.bbmpc_synchronize(self._h))

    # -- multi-GPU: one all-gather of the per-agent records per control step (include/bbmpc.h) ------
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes from rank 0 that every rank passes to comm_init (ship them over any side channel)."""
        buf = ctypes.create_string_buffer(L.COMM_ID_BYTES)
        L.check(L.lib.bbmpc_comm_unique_id(buf, L.COMM_ID_BYTES))
        return buf.raw

    def comm_init(self, unique_id, nranks, rank):
        if len(unique_id) != L.COMM_ID_BYTES:
            raise ValueError("unique_id must be %d bytes" % L.COMM_ID_BYTES)
        L.check(L.lib.bbmpc_comm_init(self._h, ctypes.c_char_p(bytes(unique_id)), int(nranks), int(rank)))

    def comm_init_local(self, group_key, nranks, rank):
        """Rank `rank` of an in-process communicator shared by the handles that pass the same key (one device, no RCCL):
        bbmpc_comm_init_local.  See parallel.attach_local_comm."""
        L.check(L.lib.bbmpc_comm_init_local(self._h, ctypes.c_uint64(int(group_key)), int(nranks), int(rank)))

    def gather_records_dev(self, d_records, d_gathered, count_per_rank, slot):
        L.check(L.lib.bbmpc_gather_records_dev(self._h, ctypes.c_void_p(d_records), ctypes.c_void_p(d_gathered),
                                               int(count_per_rank), int(slot)))

    def optimize_gather_dev(self, d_state, d_records, d_gathered, slot, t=0, add_exploration_noise=False,
                            d_next_state=0):
        L.check(L.lib.bbmpc_optimize_gather_dev(self._h, ctypes.c_void_p(d_state), int(t),
                                                int(bool(add_exploration_noise)), ctypes.c_void_p(d_records),
                                                ctypes.c_void_p(d_next_state or 0), ctypes.c_void_p(d_gathered),
                                                int(slot)))

    def graph_stats(self):
        """Host-in / host-out calls served by replaying a captured hipGraph -- bbmpc_graph_stats."""
        a = ctypes.c_int64(0)
        L.check(L.lib.bbmpc_graph_stats(self._h, ctypes.byref(a)))
        return a.value

    def call_stats(self):
        """(calls served by the resident kernel of the previous call, calls that launched) -- bbmpc_call_stats."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        L.check(L.lib.bbmpc_call_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def comm_info(self):
        """(nranks, rank, sync_mode) as the communicator itself reports them (ncclCommCount / ncclCommUserRank)."""
        n, r, m = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        L.check(L.lib.bbmpc_comm_info(self._h, ctypes.byref(n), ctypes.byref(r), ctypes.byref(m)))
        return n.value, r.value, m.value

    def optimize_gather(self, state, d_gathered, slot, t=0, add_exploration_noise=False):
        """`optimize` for this rank's agents (NumPy in / out) + the device all-gather of their records into
        d_gathered (device address of [num_agents_global, U+S+1] floats), overlapped with the next control step."""
        fast = self._fast
        if fast is None:
            fast = self._bind_fast()
        if fast:
            out = fast.optimize_gather(state, d_gathered, slot, t, add_exploration_noise)
            if out.__class__ is tuple:
                return out
            if out is not NotImplemented:
                L.check(out)
        io = self._io_buffers()
        st, action, nxt, rew, p_st, p_act, p_nxt, p_rew = io
        state = np.asarray(state)
        if state.shape != (self.A, self.S):
            raise ValueError("state must be [num_agents, dim_S] = [%d, %d], got %s" % (self.A, self.S, state.shape))
        np.copyto(st, state, casting="unsafe")
        L.check(self._lib.bbmpc_optimize_gather(self._h, p_st, int(t), 1 if add_exploration_noise else 0, p_act, p_nxt,
                                            p_rew, ctypes.c_void_p(d_gathered), int(slot)))
        return action.copy(), nxt.copy(), rew.copy()

    def gather_wait(self, slot, host_block=False):
        L.check(L.lib.bbmpc_gather_wait(self._h, int(slot), int(bool(host_block))))

    def comm_destroy(self):
        L.check(L.lib.bbmpc_comm_destroy(self._h))

    # -- hot path --------------------------------------------------------------------------
    def optimize(self, state, t=0, add_exploration_noise=False):
        # One extension call (csrc/pyfast.cpp): the observation read in place, the results allocated before the library
        # call and written by it.  It answers with the result tuple, with the library's error code, or with NotImplemented
        # for anything but a C-contiguous float32 / float64 [A, S] array and an index-like t: the body below takes those.
        fast = self._fast
        if fast is None:
            fast = self._bind_fast()
        if fast:
            out = fast.optimize(state, t, add_exploration_noise)
            if out.__class__ is tuple:
                return out
            if out is not NotImplemented:
                L.check(out)
        # persistent I/O buffers with cached ctypes pointers: building four `ndarray.ctypes` views per call costs more
        # host time (~15 us) than the H2D/D2H traffic of a control step
        st, action, nxt, rew, p_st, p_act, p_nxt, p_rew = self._io_buffers()
        state = np.asarray(state)
        if state.shape != (self.A, self.S):
            raise ValueError("state must be [num_agents, dim_S] = [%d, %d], got %s" % (self.A, self.S, state.shape))
        np.copyto(st, state, casting="unsafe")
        code = self._lib.bbmpc_optimize(self._h, p_st, int(t), 1 if add_exploration_noise else 0, p_act, p_nxt, p_rew)
        if code != 0:
            L.check(code)
        return action.copy(), nxt.copy(), rew.copy()

    def _bind_fast(self):
        """The _fastcall object of this handle (created at the first control step), or False: BBMPC_FASTCALL=0 when the
        engine was created, or no usable extension (_lib.fastcall warns once per process)."""
        fast = (L.fastcall_bind(self._lib, self._h.value, self.A, self.S, self.U) if self._fastcall_on else None) or False
        self._fast = fast
        return fast

    def _io_buffers(self):
        io = self.__dict__.get("_io")
        if io is None:
            bufs = (np.empty((self.A, self.S), np.float32), np.empty((self.A, self.U), np.float32),
                    np.empty((self.A, self.S), np.float32), np.empty((self.A,), np.float32))
            io = self._io = bufs + tuple(L.ptr(b) for b in bufs)
        return io

    def rollout_episode(self, start_state, num_steps, add_exploration_noise=False):
        """T closed-loop control steps on the device (model = environment); returns
        (actions [T,A,U], next_states [T,A,S], rewards [T,A])."""
        s = L.f32c(start_state)
        if s.shape != (self.A, self.S):
            raise ValueError("start_state must be [%d, %d]" % (self.A, self.S))
        rec = np.empty((int(num_steps), self.A, self.U + self.S + 1), np.float32)
        L.check(L.lib.bbmpc_rollout_episode(self._h, L.ptr(s), int(num_steps), int(bool(add_exploration_noise)),
                                            L.ptr(rec)))
        return rec[..., :self.U], rec[..., self.U:self.U + self.S], rec[..., self.U + self.S]

    def optimize_dev(self, d_state, d_record, t=0, add_exploration_noise=False, d_next_state=0):
        L.check(L.lib.bbmpc_optimize_dev(self._h, ctypes.c_void_p(d_state), int(t), int(bool(add_exploration_noise)),
                                         ctypes.c_void_p(d_record), ctypes.c_void_p(d_next_state or 0)))

    def evaluate(self, state, action_sequences):
        state = L.f32c(state)
        seq = L.f32c(action_sequences)
        if state.shape != (self.A, self.S):
            raise ValueError("current_states must be [%d, %d], got %s" % (self.A, self.S, state.shape))
        if seq.ndim != 4 or seq.shape[1:] != (self.A, self.H, self.U):
            raise ValueError("action_sequences must be [n, %d, %d, %d], got %s" % (self.A, self.H, self.U, seq.shape))
        n = seq.shape[0]
        out = np.empty((n, self.A), np.float32)
        if n == 0:
            return out
        L.check(L.lib.bbmpc_evaluate(self._h, L.ptr(state), L.ptr(seq), n, L.ptr(out)))
        return out

    def evaluate_dev(self, d_state, d_seq, n_pop, d_rewards):
        L.check(L.lib.bbmpc_evaluate_dev(self._h, ctypes.c_void_p(d_state), ctypes.c_void_p(d_seq), int(n_pop),
                                         ctypes.c_void_p(d_rewards)))

    def set_particles(self, num_particles, process_noise_std=None, risk_kappa=0.0):
        """Particle trajectory evaluation (bbmpc_set_particles): every candidate is rolled out `num_particles` times with
        additive N(0, process_noise_std^2) noise on the predicted next state ([dim_S] or a scalar) and scored
        mean - risk_kappa * std of the returns.  0 switches back to the deterministic paths."""
        p = int(num_particles)
        if p == 0:
            L.check(L.lib.bbmpc_set_particles(self._h, 0, None, ctypes.c_float(0.0)))
            self.P = 0
            return
        if process_noise_std is None:
            raise ValueError("process_noise_std is required with num_particles > 0")
        sg = np.asarray(process_noise_std, np.float32)
        sg = L.f32c(np.full((self.S,), sg, np.float32) if sg.ndim == 0 else sg.reshape(-1))
        if sg.shape != (self.S,):
            raise ValueError("process_noise_std must be a scalar or [dim_S] = [%d], got %s" % (self.S, sg.shape))
        L.check(L.lib.bbmpc_set_particles(self._h, p, L.ptr(sg), ctypes.c_float(float(risk_kappa))))
        self.P = p

    def set_particle_risk(self, kind=L.RISK_MEAN_STD, tail_count=0):
        """How the particle returns become the score (bbmpc_set_particle_risk): RISK_MEAN_STD (tail_count 0) is
        mean - risk_kappa * std; RISK_CVAR is the mean of the `tail_count` worst returns, 1 <= tail_count <= num_particles
        (1: the worst case over the particles).  Handle state, before or after set_particles."""
        L.check(L.lib.bbmpc_set_particle_risk(self._h, int(kind), int(tail_count)))
        self.risk = (int(kind), int(tail_count))

    def set_chance_constraint(self, lo, hi, max_violation=0.0, weight=1e3):
        """Chance constraint of the particle evaluator (bbmpc_set_chance_constraint): a state box [lo, hi] ([dim_S] each,
        -inf / +inf = unbounded) that does not end a rollout; a candidate's score loses
        weight * max(0, v - max_violation), v the share of its particles that ever leave the box.  Needs a DYN_MLP handle
        with particles on and a built-in or HIP-source reward.  lo = hi = None removes it."""
        bounds = []
        for b in (lo, hi):
            if b is not None:
                b = L.f32c(np.asarray(b, np.float32).reshape(-1))
                if b.shape != (self.S,):         # the C side reads dim_S floats from this buffer
                    raise ValueError("a state bound must be [%d], got %s" % (self.S, b.shape))
            bounds.append(b)
        L.check(L.lib.bbmpc_set_chance_constraint(self._h, L.ptr(bounds[0]), L.ptr(bounds[1]), ctypes.c_float(float(max_violation)),
                                                  ctypes.c_float(float(weight))))

    def clear_chance_constraint(self):
        L.check(L.lib.bbmpc_set_chance_constraint(self._h, None, None, ctypes.c_float(0.0), ctypes.c_float(0.0)))

    def constraint_violations(self, n_pop=None, first_steps=False):
        """v of the most recent particle rollout (bbmpc_get_constraint_violations): float32 [n_pop, A], the share of each
        candidate's particles that left the box; with first_steps also int32 [n_pop, P, A], the first step in 1 .. H
        outside the box, 0 = never.  n_pop: the candidates of that rollout -- by default what the handle says it rolled
        out (bbmpc_get_state "constraint_shape")."""
        n = int(n_pop if n_pop is not None else self.get_state("constraint_shape", (4,))[0])
        prob = np.empty((max(n, 0), self.A), np.float32)
        first = np.empty((max(n, 0), max(int(getattr(self, "P", 0)), 1), self.A), np.int32) if first_steps else None
        L.check(L.lib.bbmpc_get_constraint_violations(self._h, n, L.ptr(prob), L.ptr(first)))
        return (prob, first) if first_steps else prob

    def evaluate_particles(self, state, action_sequences, want_returns=True):
        """(scores [n, A], per-particle returns [n, P, A] or None) -- bbmpc_evaluate_particles."""
        state = L.f32c(state)
        seq = L.f32c(action_sequences)
        if state.shape != (self.A, self.S):
            raise ValueError("current_states must be [%d, %d], got %s" % (self.A, self.S, state.shape))
        if seq.ndim != 4 or seq.shape[1:] != (self.A, self.H, self.U):
            raise ValueError("action_sequences must be [n, %d, %d, %d], got %s" % (self.A, self.H, self.U, seq.shape))
        p = getattr(self, "P", 0)
        if p <= 0:
            raise ValueError("particles are off: call set_particles first")
        n = seq.shape[0]
        scores = np.empty((n, self.A), np.float32)
        returns = np.empty((n, p, self.A), np.float32) if want_returns else None
        if n:
            L.check(L.lib.bbmpc_evaluate_particles(self._h, L.ptr(state), L.ptr(seq), n, L.ptr(scores), L.ptr(returns)))
        return scores, returns

    def evaluate_particles_dev(self, d_state, d_seq, n_pop, d_scores, d_returns=0):
        L.check(L.lib.bbmpc_evaluate_particles_dev(self._h, ctypes.c_void_p(d_state), ctypes.c_void_p(d_seq), int(n_pop),
                                                   ctypes.c_void_p(d_scores), ctypes.c_void_p(d_returns or 0)))

    def predict_next_state(self, states, actions):
        states, actions = L.f32c(states), L.f32c(actions)
        b = states.shape[0]
        if states.shape != (b, self.S) or actions.shape != (b, self.U):
            raise ValueError("states [B,%d] / actions [B,%d] expected" % (self.S, self.U))
        out = np.empty((b, self.S), np.float32)
        if b:
            L.check(L.lib.bbmpc_predict_next_state(self._h, L.ptr(states), L.ptr(actions), b, L.ptr(out)))
        return out

    def evaluate_next_reward(self, states, next_states, actions):
        states, next_states, actions = L.f32c(states), L.f32c(next_states), L.f32c(actions)
        b = states.shape[0] if states.ndim == 2 else -1
        # the C side copies b*S / b*S / b*U floats from these buffers: a wrong shape must not become an out-of-bounds read
        if states.shape != (b, self.S) or next_states.shape != (b, self.S) or actions.shape != (b, self.U):
            raise ValueError("states / next_states [B,%d] and actions [B,%d] expected, got %s, %s, %s"
                             % (self.S, self.U, states.shape, next_states.shape, actions.shape))
        out = np.empty((b,), np.float32)
        if b:
            L.check(L.lib.bbmpc_evaluate_next_reward(self._h, L.ptr(states), L.ptr(next_states), L.ptr(actions), b,
                                                     L.ptr(out)))
        return out

    def step_dev(self, d_states, d_actions, action_stride, batch, d_next_states, d_rewards=0):
        L.check(L.lib.bbmpc_step_dev(self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_actions),
                                     int(action_stride), int(batch), ctypes.c_void_p(d_next_states),
                                     ctypes.c_void_p(d_rewards or 0)))

    def predict_trajectories(self, states, action_sequences, want_states=True, want_rewards=True):
        """Open-loop prediction (bbmpc_predict_trajectories): states [B,S], action_sequences [B,Hq,U] ->
        (states [B,Hq,S], rewards [B,Hq]); s_{t+1} = predict_next_state(s_t, a_t) from each row's own start, every state
        and reward kept.  Hq is free of the handle's planning horizon.  An output that is not wanted comes back None."""
        states, seq = L.f32c(states), L.f32c(action_sequences)
        b = states.shape[0] if states.ndim == 2 else -1
        # the C side copies b*S and b*Hq*U floats from these buffers: a wrong shape must not become an out-of-bounds read
        if states.shape != (b, self.S) or seq.ndim != 3 or seq.shape[0] != b or seq.shape[2] != self.U:
            raise ValueError("states [B,%d] and action_sequences [B,Hq,%d] expected, got %s, %s"
                             % (self.S, self.U, states.shape, seq.shape))
        hq = seq.shape[1]
        out_s = np.empty((b, hq, self.S), np.float32) if want_states else None
        out_r = np.empty((b, hq), np.float32) if want_rewards else None
        L.check(L.lib.bbmpc_predict_trajectories(self._h, L.ptr(states), L.ptr(seq), b, hq, L.ptr(out_s), L.ptr(out_r)))
        return out_s, out_r

    def predict_trajectories_dev(self, d_states, d_action_sequences, batch, horizon, d_states_out=0, d_rewards_out=0):
        """The same on device addresses, enqueued on the handle's stream (either output may be 0, not both)."""
        L.check(L.lib.bbmpc_predict_trajectories_dev(self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_action_sequences),
                                                     int(batch), int(horizon), ctypes.c_void_p(d_states_out or 0),
                                                     ctypes.c_void_p(d_rewards_out or 0)))

    def plan_gradient(self, states, action_sequences, want_returns=True):
        """Plan gradients (bbmpc_plan_gradient): states [B,S], action_sequences [B,Hq,U] -> (returns [B], grad [B,Hq,U]) with
        R[b] = sum_t r(s_t, a_t, s_{t+1}) + terminal_weight * V(s_Hq) through the learned dynamics, the learned reward and
        (when installed) the learned terminal value, and grad[b,t,u] = dR[b] / da_t[u].  Actions are used as given.  A rows
        call: Hq is free of the handle's planning horizon.  returns comes back None when it is not wanted."""
        states, seq = L.f32c(states), L.f32c(action_sequences)
        b = states.shape[0] if states.ndim == 2 else -1
        # the C side copies b*S and b*Hq*U floats from these buffers: a wrong shape must not become an out-of-bounds read
        if states.shape != (b, self.S) or seq.ndim != 3 or seq.shape[0] != b or seq.shape[2] != self.U:
            raise ValueError("states [B,%d] and action_sequences [B,Hq,%d] expected, got %s, %s"
                             % (self.S, self.U, states.shape, seq.shape))
        hq = seq.shape[1]
        out_r = np.empty((b,), np.float32) if want_returns else None
        out_g = np.empty((b, hq, self.U), np.float32)
        L.check(L.lib.bbmpc_plan_gradient(self._h, L.ptr(states), L.ptr(seq), b, hq, L.ptr(out_r), L.ptr(out_g)))
        return out_r, out_g

    def plan_gradient_dev(self, d_states, d_action_sequences, batch, horizon, d_returns_out, d_grad_out):
        """The same on device addresses, enqueued on the handle's stream (d_returns_out may be 0)."""
        L.check(L.lib.bbmpc_plan_gradient_dev(self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_action_sequences), int(batch),
                                              int(horizon), ctypes.c_void_p(d_returns_out or 0), ctypes.c_void_p(d_grad_out)))

    REFINE_METHODS = {"adam": 0, "sgd": 1}

    def refine_plans(self, states, plans, steps, lr, method="adam", keep_best=True):
        """Plan refinement on the device (bbmpc_refine_plans): `steps` projected ascent steps ("adam" or "sgd", step size
        lr, clipped to the handle's action bounds) on the model return of plan_gradient, the whole loop on the handle's
        stream.  states [B,S], plans [B,Hq,U] -> (plans [B,Hq,U] float32, returns [B]).  keep_best: per row the best plan
        by model return, the input included, and its return; otherwise the last iterate and its return."""
        if method not in self.REFINE_METHODS:
            raise ValueError("method must be 'adam' or 'sgd', got %r" % (method,))
        states = L.f32c(states)
        seq = np.array(plans, np.float32, order="C")            # a copy: the C side refines it in place
        b = states.shape[0] if states.ndim == 2 else -1
        if states.shape != (b, self.S) or seq.ndim != 3 or seq.shape[0] != b or seq.shape[2] != self.U:
            raise ValueError("states [B,%d] and plans [B,Hq,%d] expected, got %s, %s" % (self.S, self.U, states.shape, seq.shape))
        out_r = np.empty((b,), np.float32)
        L.check(L.lib.bbmpc_refine_plans(self._h, L.ptr(states), L.ptr(seq), b, seq.shape[1], int(steps), float(lr),
                                         self.REFINE_METHODS[method], 1 if keep_best else 0, L.ptr(out_r)))
        return seq, out_r

    def refine_plans_dev(self, d_states, d_plans, batch, horizon, steps, lr, method="adam", keep_best=True, d_returns_out=0):
        """The same on device addresses, enqueued on the handle's stream: d_plans is refined in place (d_returns_out may be 0)."""
        if method not in self.REFINE_METHODS:
            raise ValueError("method must be 'adam' or 'sgd', got %r" % (method,))
        L.check(L.lib.bbmpc_refine_plans_dev(self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_plans), int(batch), int(horizon),
                                             int(steps), float(lr), self.REFINE_METHODS[method], 1 if keep_best else 0,
                                             ctypes.c_void_p(d_returns_out or 0)))

    def set_grad_refine(self, steps, lr=0.05, method="adam", candidates=0):
        """Gradient steps on CEM's candidates (bbmpc_set_grad_refine): in every iteration the last `candidates` columns of
        every agent (0: all) take `steps` steps of refine_plans_dev(keep_best=False) before the rollout scores them.
        steps = 0 switches it off."""
        if method not in self.REFINE_METHODS:
            raise ValueError("method must be 'adam' or 'sgd', got %r" % (method,))
        L.check(L.lib.bbmpc_set_grad_refine(self._h, int(steps), float(lr), self.REFINE_METHODS[method], int(candidates)))

    def get_grad_refine(self):
        """(steps, lr, method, candidates) of set_grad_refine; steps = 0 while it is off."""
        s, m, c, lr = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_float()
        L.check(L.lib.bbmpc_get_grad_refine(self._h, ctypes.byref(s), ctypes.byref(lr), ctypes.byref(m), ctypes.byref(c)))
        return s.value, lr.value, "sgd" if m.value == 1 else "adam", c.value

    def predict_trajectory_particles(self, states, action_sequences, eps=None, want_particles=False, quantile_ranks=None):
        """Trajectory distributions (bbmpc_predict_trajectory_particles): states [B,S], action_sequences [B,Hq,U] ->
        (state_mean [B,Hq,S], state_std [B,Hq,S], reward_mean [B,Hq], reward_std [B,Hq]) over the P particles of
        set_particles, each rolled with process noise (and the ensemble member / log-variance head it follows) from the
        row's own start state; with want_particles also (particle_states [B,P,Hq,S], particle_rewards [B,P,Hq]).
        eps: standard normals [B,P,Hq,S], or None for the handle's own draws.  quantile_ranks: up to 8 ranks in [0, P) --
        then (bbmpc_predict_trajectory_quantiles) state_quantiles [B,L,Hq,S] and reward_quantiles [B,L,Hq] follow the
        moments (and precede the particle tensors): for rank r the particle value whose stable rank among the P particles
        of that element is r (0: the minimum, P - 1: the maximum)."""
        states, seq = L.f32c(states), L.f32c(action_sequences)
        b = states.shape[0] if states.ndim == 2 else -1
        # the C side copies b*S, b*Hq*U and b*P*Hq*S floats from these buffers: a wrong shape must not become an out-of-bounds read
        if states.shape != (b, self.S) or seq.ndim != 3 or seq.shape[0] != b or seq.shape[2] != self.U:
            raise ValueError("states [B,%d] and action_sequences [B,Hq,%d] expected, got %s, %s"
                             % (self.S, self.U, states.shape, seq.shape))
        p = getattr(self, "P", 0)
        if p <= 0:
            raise ValueError("particles are off: call set_particles first")
        hq = seq.shape[1]
        if eps is not None:
            eps = L.f32c(eps)
            if eps.shape != (b, p, hq, self.S):
                raise ValueError("eps must be [B, P, Hq, dim_S] = [%d, %d, %d, %d], got %s" % (b, p, hq, self.S, eps.shape))
        outs = [np.empty((b, hq, self.S), np.float32), np.empty((b, hq, self.S), np.float32),
                np.empty((b, hq), np.float32), np.empty((b, hq), np.float32)]
        parts = [np.empty((b, p, hq, self.S), np.float32), np.empty((b, p, hq), np.float32)] if want_particles else []
        pptrs = [L.ptr(o) for o in parts] or [None, None]
        if quantile_ranks is None:
            L.check(L.lib.bbmpc_predict_trajectory_particles(self._h, L.ptr(states), L.ptr(seq), b, hq, L.ptr(eps),
                                                             *([L.ptr(o) for o in outs] + pptrs)))
            return tuple(outs + parts)
        ranks = np.ascontiguousarray(np.asarray(quantile_ranks).reshape(-1), np.int32)
        nl = ranks.size
        if not 1 <= nl <= L.MAX_QUANTILE_LEVELS:           # (the C side sizes its copies by num_levels: refuse before it)
            raise ValueError("quantile_ranks must hold 1 to %d ranks, got %d" % (L.MAX_QUANTILE_LEVELS, nl))
        quants = [np.empty((b, nl, hq, self.S), np.float32), np.empty((b, nl, hq), np.float32)]
        L.check(L.lib.bbmpc_predict_trajectory_quantiles(self._h, L.ptr(states), L.ptr(seq), b, hq, L.ptr(eps),
                                                         *([L.ptr(o) for o in outs] + pptrs + [nl, ranks.ctypes.data_as(ctypes.c_void_p)]
                                                           + [L.ptr(o) for o in quants])))
        return tuple(outs + quants + parts)

    def predict_trajectory_particles_dev(self, d_states, d_action_sequences, batch, horizon, d_eps=0, d_state_mean=0,
                                         d_state_std=0, d_reward_mean=0, d_reward_std=0, d_particle_states=0,
                                         d_particle_rewards=0):
        """The same on device addresses, enqueued on the handle's stream (any output may be 0, not all six; d_eps = 0: the
        handle's own draws)."""
        L.check(L.lib.bbmpc_predict_trajectory_particles_dev(
            self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_action_sequences), int(batch), int(horizon),
            *[ctypes.c_void_p(v or 0) for v in (d_eps, d_state_mean, d_state_std, d_reward_mean, d_reward_std,
                                                d_particle_states, d_particle_rewards)]))

    def predict_trajectory_quantiles_dev(self, d_states, d_action_sequences, batch, horizon, quantile_ranks, d_eps=0,
                                         d_state_mean=0, d_state_std=0, d_reward_mean=0, d_reward_std=0, d_particle_states=0,
                                         d_particle_rewards=0, d_state_quantiles=0, d_reward_quantiles=0):
        """bbmpc_predict_trajectory_quantiles_dev on device addresses (any output may be 0, not all eight); quantile_ranks
        is a host sequence."""
        ranks = np.ascontiguousarray(np.asarray(quantile_ranks).reshape(-1), np.int32)
        L.check(L.lib.bbmpc_predict_trajectory_quantiles_dev(
            self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_action_sequences), int(batch), int(horizon),
            *([ctypes.c_void_p(v or 0) for v in (d_eps, d_state_mean, d_state_std, d_reward_mean, d_reward_std,
                                                 d_particle_states, d_particle_rewards)]
              + [int(ranks.size), ranks.ctypes.data_as(ctypes.c_void_p)]
              + [ctypes.c_void_p(d_state_quantiles or 0), ctypes.c_void_p(d_reward_quantiles or 0)])))

    def set_sampling_correlation(self, matrix):
        """Temporally correlated sampling for CEM / PI2 (bbmpc_set_sampling_correlation): `matrix` is the [H, H] mixing
        matrix applied along the time axis of the standard draws (utils/colored_noise.py builds the usual ones); None
        removes it.  While one is installed control steps take the per-iteration launch paths, as with set_trace."""
        if matrix is None:
            L.check(L.lib.bbmpc_set_sampling_correlation(self._h, None, 0))
            return
        m = L.f32c(matrix)
        L.check(L.lib.bbmpc_set_sampling_correlation(self._h, L.ptr(m), int(m.size)))

    def sampling_correlation_installed(self):
        """True while a mixing matrix is installed (bbmpc_get_sampling_correlation)."""
        v = ctypes.c_int32(0)
        L.check(L.lib.bbmpc_get_sampling_correlation(self._h, ctypes.byref(v)))
        return bool(v.value)

    def set_elite_carry(self, keep, shift):
        """Elite carry-over for CEM (bbmpc_set_elite_carry): the best `keep` elites of an iteration replace the last
        candidates of the next one, the best `shift` elites of a control step's last iteration, moved one planning step
        forward, those of the next control step's first iteration.  (0, 0) switches it off.  While it is on control steps
        take the per-iteration launch paths, as with set_trace."""
        L.check(L.lib.bbmpc_set_elite_carry(self._h, int(keep), int(shift)))

    def elite_carry(self):
        """(keep, shift, stored): the setting and the number of elites held for the next control step
        (bbmpc_get_elite_carry)."""
        v = [ctypes.c_int(0) for _ in range(3)]
        L.check(L.lib.bbmpc_get_elite_carry(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def set_policy_prior_mlp(self, weights, biases, activations, stats=None, count=1, noise_std=0.0):
        """Learned policy prior of a CEM + DYN_MLP handle (bbmpc_set_policy_prior_mlp): Dense kernels [in, out] / biases
        [out] from dim_S inputs to dim_U outputs, any ACT_* code per layer; stats = (mean_in [S], std_in [S], mean_out [U],
        std_out [U]) or None.  `count` closed-loop rollouts of the policy through the learned model, with N(0, noise_std^2)
        added to every action, replace that many sampled candidates of every iteration.  weights = None (or an empty list)
        removes the network."""
        if not weights:
            L.check(L.lib.bbmpc_set_policy_prior_mlp(self._h, 0, None, None, None, None, 0, None, 0, 0.0))
            return
        n = len(weights)
        ws = [L.f32c(w) for w in weights]
        bs = [L.f32c(np.asarray(b).reshape(-1)) for b in biases]
        dims = [ws[0].shape[0]] + [w.shape[1] for w in ws]
        for i, (w, b) in enumerate(zip(ws, bs)):
            if w.ndim != 2 or w.shape[0] != dims[i] or b.shape != (w.shape[1],):
                raise ValueError("layer %d: kernel must be [in,out] and bias [out]" % i)
        dims_a = (ctypes.c_int32 * (n + 1))(*dims)
        acts_a = (ctypes.c_int32 * n)(*[int(a) for a in activations])
        wp = (ctypes.c_void_p * n)(*[w.ctypes.data for w in ws])
        bp = (ctypes.c_void_p * n)(*[b.ctypes.data for b in bs])
        sp = None
        if stats is not None:
            st = [L.f32c(np.asarray(s).reshape(-1)) for s in stats]
            if [s.shape for s in st] != [(dims[0],), (dims[0],), (dims[-1],), (dims[-1],)]:
                raise ValueError("stats must be (mean_in [%d], std_in [%d], mean_out [%d], std_out [%d])"
                                 % (dims[0], dims[0], dims[-1], dims[-1]))
            sp = (ctypes.c_void_p * 4)(*[s.ctypes.data for s in st])
        L.check(L.lib.bbmpc_set_policy_prior_mlp(self._h, n, dims_a, acts_a, wp, bp, 1 if stats is not None else 0, sp,
                                                 int(count), float(noise_std)))

    def policy_prior(self):
        """(count, noise_std) of the installed policy prior (bbmpc_get_policy_prior); BBMPCError (state) without one."""
        c, s = ctypes.c_int32(0), ctypes.c_float(0.0)
        L.check(L.lib.bbmpc_get_policy_prior(self._h, ctypes.byref(c), ctypes.byref(s)))
        return int(c.value), float(s.value)

    def evaluate_policy_prior(self, states):
        """pi on rows (bbmpc_evaluate_policy_prior): states [B, S] -> actions [B, U], no noise and no clip."""
        states = L.f32c(states)
        b = states.shape[0] if states.ndim == 2 else -1
        if states.shape != (b, self.S):                  # the C side copies b * S floats from this buffer
            raise ValueError("states [B,%d] expected, got %s" % (self.S, states.shape))
        out = np.empty((b, self.U), np.float32)
        if b:
            L.check(L.lib.bbmpc_evaluate_policy_prior(self._h, L.ptr(states), b, L.ptr(out)))
        return out

    def evaluate_policy_prior_dev(self, d_states, batch, d_actions):
        L.check(L.lib.bbmpc_evaluate_policy_prior_dev(self._h, ctypes.c_void_p(d_states), int(batch), ctypes.c_void_p(d_actions)))

    def predict_policy_rollouts(self, states, noise=None, want_actions=True, want_states=True):
        """The K policy rollouts of every agent (bbmpc_predict_policy_rollouts), by the kernel the control step runs:
        states [A, S], noise [A, K, H, U] standard normals or None (the handle's own stream at the current control step,
        iteration 0) -> (actions [K, A, H, U], states [K, A, H, S]); an output not wanted is None."""
        states = L.f32c(states)
        if states.shape != (self.A, self.S):
            raise ValueError("states [%d,%d] expected, got %s" % (self.A, self.S, states.shape))
        k = self.policy_prior()[0]
        if not (want_actions or want_states):
            raise ValueError("at least one of want_actions / want_states")
        nz = None
        if noise is not None:
            nz = L.f32c(noise)
            if nz.shape != (self.A, k, self.H, self.U):
                raise ValueError("noise [%d,%d,%d,%d] expected, got %s" % (self.A, k, self.H, self.U, nz.shape))
        acts = np.empty((k, self.A, self.H, self.U), np.float32) if want_actions else None
        sts = np.empty((k, self.A, self.H, self.S), np.float32) if want_states else None
        L.check(L.lib.bbmpc_predict_policy_rollouts(self._h, L.ptr(states), L.ptr(nz) if nz is not None else None,
                                                    L.ptr(acts) if acts is not None else None,
                                                    L.ptr(sts) if sts is not None else None))
        return acts, sts

    def predict_policy_rollouts_dev(self, d_states, d_noise=0, d_actions_out=0, d_states_out=0):
        """Device pointers (0 = NULL), enqueued on the handle's stream (bbmpc_predict_policy_rollouts_dev)."""
        L.check(L.lib.bbmpc_predict_policy_rollouts_dev(self._h, ctypes.c_void_p(d_states), ctypes.c_void_p(d_noise or None),
                                                        ctypes.c_void_p(d_actions_out or None), ctypes.c_void_p(d_states_out or None)))

    def set_keep_plan(self, enabled=True):
        """Opt-in switch of plan readback (bbmpc_set_keep_plan): the control steps that follow keep their solution in HBM
        (the routing of set_trace: same results, slower paths).  Off by default."""
        L.check(L.lib.bbmpc_set_keep_plan(self._h, int(bool(enabled))))

    def get_plan(self):
        """The action sequence [A,H,U] the last control step took its action from (bbmpc_get_plan)."""
        out = np.empty((self.A, self.H, self.U), np.float32)
        L.check(L.lib.bbmpc_get_plan(self._h, L.ptr(out)))
        return out

    def trajectory_sq_error_dev(self, d_predicted, d_observed, batch, horizon, d_sum_sq):
        """d_sum_sq (float64 [Hq*S]) = sum over rows of (predicted - observed)^2, device arrays [B,Hq,S]; deterministic."""
        L.check(L.lib.bbmpc_trajectory_sq_error_dev(self._h, ctypes.c_void_p(d_predicted), ctypes.c_void_p(d_observed),
                                                    int(batch), int(horizon), ctypes.c_void_p(d_sum_sq)))

    # -- parity hooks ----------------------------------------------------------------------
    def inject_noise(self, kind, data):
        if data is None:
            L.check(L.lib.bbmpc_inject_noise(self._h, int(kind), None, 0))
            return
        d = L.f32c(data)
        L.check(L.lib.bbmpc_inject_noise(self._h, int(kind), L.ptr(d), d.size))

    def dump_noise(self, kind, control_step, iteration, shape):
        out = np.empty(shape, np.float32)
        L.check(L.lib.bbmpc_dump_noise(self._h, int(kind), int(control_step), int(iteration), L.ptr(out), out.size))
        return out

    def set_trace(self, enabled=True):
        L.check(L.lib.bbmpc_set_trace(self._h, int(bool(enabled))))

    def get_trace(self, iteration, item):
        if item == L.TRACE_REWARDS:
            out = np.empty(((2 if self.cfg.optimizer == L.OPT_SPSA else 1) * self.N, self.A), np.float32)
        elif item in (L.TRACE_MEAN, L.TRACE_VAR):
            out = np.empty((self.A, self.H, self.U), np.float32)
        elif item == L.TRACE_ELITES:
            if self.cfg.optimizer == L.OPT_CEM:
                out = np.empty((self.A, self.k), np.int32)
            elif self.cfg.optimizer == L.OPT_CMAES:
                groups = self.A if (self.cfg.quirks & L.CMAES_PER_AGENT) else 1
                out = np.empty((groups, self.k), np.int32)
            else:
                out = np.empty((self.A,), np.int32)
        elif item == L.TRACE_TOPK_PASSES:
            out = np.empty((self.A,), np.int32)
        elif item == L.TRACE_SAMPLES:
            out = np.empty((self.N, self.A, self.H, self.U), np.float32)
        elif item in (L.TRACE_CMA_B, L.TRACE_CMA_C, L.TRACE_CMA_D):
            per_agent = bool(self.cfg.quirks & L.CMAES_PER_AGENT)
            groups = self.A if per_agent else 1
            n = self.H * self.U * (1 if per_agent else self.A)
            out = np.empty((groups, n) if item == L.TRACE_CMA_D else (groups, n, n), np.float32)
        elif item == L.TRACE_CMA_SVD_STATS:
            out = np.empty((self.A if (self.cfg.quirks & L.CMAES_PER_AGENT) else 1, 16), np.int32)
        else:
            raise ValueError(item)
        L.check(L.lib.bbmpc_get_trace(self._h, int(iteration), int(item), L.ptr(out), out.nbytes))
        return out

    def get_state(self, name, shape=None):
        out = np.empty(shape if shape is not None else (self.A, self.H, self.U), np.float32)
        L.check(L.lib.bbmpc_get_state(self._h, name.encode(), L.ptr(out), out.size))
        return out

    def set_state(self, name, data):
        d = L.f32c(data)
        L.check(L.lib.bbmpc_set_state(self._h, name.encode(), L.ptr(d), d.size))

    # -- measurement -----------------------------------------------------------------------
    def set_profiling(self, enabled=True, every=1):
        """HIP events around every `every`-th launch of the dominant kernel (see include/bbmpc.h)."""
        L.check(L.lib.bbmpc_set_profiling(self._h, (max(int(every), 1) if enabled else 0)))

    def get_profile(self):
        ms, n, name = ctypes.c_double(), ctypes.c_int64(), ctypes.c_char_p()
        L.check(L.lib.bbmpc_get_profile(self._h, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(name)))
        return ms.value, n.value, (name.value or b"").decode()

    def profile_instantiation(self):
        """The dominant kernel with its template arguments, as rocprofv3 names it minus "void " (include/bbmpc.h)."""
        name = ctypes.c_char_p()
        L.check(L.lib.bbmpc_profile_instantiation(self._h, ctypes.byref(name)))
        return (name.value or b"").decode()
