/*
 * bbmpc.h -- C ABI of the MI355X-native sampling-MPC rollout engine.
 *
 * The reference (ossamaAhmed/blackbox_mpc v0.3) has no FFI: its hot path is a
 * Python class API that hands one tf.function graph call per control step to
 * TensorFlow.  This header declares what a maintainer of the reference would
 * bind (ctypes stub in INTEGRATION.md) to replace that graph call.  Each entry
 * point cites the reference interface it stands in for; paths are relative to
 * /root/reference/blackbox_mpc/.
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success or a negative
 *     BBMPC_E_* code; bbmpc_last_error() gives the message for the calling thread.
 *   - host-pointer entry points are synchronous: outputs are valid on return.
 *     *_dev entry points take device (HBM) pointers, enqueue on the handle's
 *     stream and return immediately.
 *   - the caller owns every buffer it passes; the handle owns device memory,
 *     stream, events.  One handle = one caller thread at a time (the reference's
 *     optimizers hold mutable tf.Variable state and are not re-entrant either).
 *   - tensors are float32, C-contiguous, in the reference's layouts:
 *       states [A,S], action sequences [N,A,H,U], rewards [N,A].
 *   - there is NO CPU fallback: every compute entry point fails with
 *     BBMPC_E_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef BBMPC_H
#define BBMPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BBMPC_ABI_VERSION 4

/* ---- status codes ------------------------------------------------------- */
#define BBMPC_OK              0
#define BBMPC_E_INVALID      -1   /* bad argument / unsupported configuration */
#define BBMPC_E_NO_DEVICE    -2   /* no usable HIP device                      */
#define BBMPC_E_HIP          -3   /* a HIP runtime call failed                 */
#define BBMPC_E_STATE        -4   /* call sequence error (e.g. MLP weights not set) */
#define BBMPC_E_UNSUPPORTED  -5   /* valid in the reference, not built yet     */

/* ---- enums -------------------------------------------------------------- */
/* optimizers/: random_search.py, cem.py, pi2.py, pso.py, cma_es.py, spsa.py */
#define BBMPC_OPT_NONE          0   /* evaluator-only handle */
#define BBMPC_OPT_RANDOM_SEARCH 1
#define BBMPC_OPT_CEM           2
#define BBMPC_OPT_PI2           3
#define BBMPC_OPT_PSO           4
#define BBMPC_OPT_CMAES         5
#define BBMPC_OPT_SPSA          6

/* dynamics plugin: utils/pendulum.py:38-92 | dynamics_functions/deterministic_mlp.py:5-51 */
#define BBMPC_DYN_PENDULUM 1
#define BBMPC_DYN_MLP      2
#define BBMPC_DYN_USER     3   /* caller-supplied: HIP source (bbmpc_set_dynamics_source) or a device-memory callback */

/* reward plugin: utils/pendulum.py:10-35 | tutorials/mujoco/cost_func.py:5-22 */
#define BBMPC_REW_PENDULUM 1
#define BBMPC_REW_CHEETAH  2
#define BBMPC_REW_USER     3   /* caller-supplied: HIP source (bbmpc_set_reward_source) or a device-memory callback */
#define BBMPC_REW_MLP      4   /* learned: a reward network (bbmpc_set_reward_mlp); with BBMPC_DYN_MLP only */

/* Dense activations (tutorials use tf.math.tanh and None); the TF 2.0 definitions, fixed slopes and constants */
#define BBMPC_ACT_NONE         0
#define BBMPC_ACT_TANH         1
#define BBMPC_ACT_RELU         2
#define BBMPC_ACT_SIGMOID      3
#define BBMPC_ACT_ELU          4   /* x > 0 ? x : e^x - 1 (alpha 1) */
#define BBMPC_ACT_SELU         5   /* lambda * (x > 0 ? x : alpha (e^x - 1)) */
#define BBMPC_ACT_SOFTPLUS     6   /* log(1 + e^x) */
#define BBMPC_ACT_SOFTSIGN     7   /* x / (1 + |x|) */
#define BBMPC_ACT_EXPONENTIAL  8   /* e^x */
#define BBMPC_ACT_HARD_SIGMOID 9   /* clip(0.2 x + 0.5, 0, 1) (Keras 2.0) */
#define BBMPC_ACT_SWISH        10  /* x * sigmoid(x) (= silu) */
#define BBMPC_ACT_LEAKY_RELU   11  /* x >= 0 ? x : 0.2 x (tf.nn.leaky_relu's default slope) */
#define BBMPC_ACT_RELU6        12  /* min(max(x, 0), 6) */

/* quirk switches; a set bit OPTS OUT of the reference's as-executed behaviour
 * (SURVEY.md section 8 quirk register).  Default 0 = bug-compatible. */
#define BBMPC_FIX_Q1_REWARD_ARG_ORDER   (1u << 0)  /* pendulum reward uses actions, not next_state */
#define BBMPC_FIX_Q2_CEM_WARM_START     (1u << 1)  /* CEM keeps shifted mean across control steps  */
#define BBMPC_FIX_Q7_EXPL_NOISE_ZERO_MEAN (1u << 2)
#define BBMPC_CMAES_PER_AGENT           (1u << 8)  /* independent CMA-ES per agent (deviation, shards) */
#define BBMPC_STRICT_MATH               (1u << 9)  /* pendulum rollouts op-for-op as the reference (atan2/sincos every
                                                      step) instead of carrying the angle; same tolerances, slower */

/* noise kinds for bbmpc_inject_noise (standard draws, reference layout) */
#define BBMPC_NOISE_TRUNC_NORMAL 1  /* [iters][N,A,H,U] unit normal, |z|<2: cem.py:90 pi2.py:65 */
#define BBMPC_NOISE_UNIFORM      2  /* [N,A,H,U] U[0,1): random_search.py:40                     */
#define BBMPC_NOISE_RADEMACHER   3  /* [iters][N,A,H,U] +-1: spsa.py:73-75                        */
#define BBMPC_NOISE_NORMAL       4  /* CMA-ES [iters][N,n] N(0,1): cma_es.py:139                  */
#define BBMPC_NOISE_PSO_SCALARS  5  /* [iters][2] N(0,1): pso.py:107-109                          */
#define BBMPC_NOISE_PSO_RESEED_TRUNC   6  /* [N,A,H,U]: pso.py:121-127 */
#define BBMPC_NOISE_PSO_RESEED_UNIFORM 7  /* [N,A,H,U]: pso.py:130-131 */
#define BBMPC_NOISE_PSO_RESET_POS      8  /* [N,A,H,U]: pso.py:147-149 */
#define BBMPC_NOISE_PSO_RESET_VEL      9  /* [N,A,H,U]: pso.py:151-152 */
#define BBMPC_NOISE_EXPLORATION       10  /* [A,U] unit trunc normal: optimizer_base.py:83-86 */
#define BBMPC_NOISE_PROCESS           11  /* [iters][A,P,H,S] N(0,1) ([A,P,H,S] on evaluator-only handles): bbmpc_set_particles */
#define BBMPC_NOISE_POLICY            12  /* [iters][A,K,H,U] N(0,1): bbmpc_set_policy_prior_mlp */

/* trace items for bbmpc_get_trace (per-iteration parity data) */
#define BBMPC_TRACE_REWARDS 1   /* [N,A]  (SPSA: [2N,A], plus then minus)   */
#define BBMPC_TRACE_MEAN    2   /* [A,H,U] distribution mean / solution after the iteration */
#define BBMPC_TRACE_VAR     3   /* [A,H,U] (CEM)                             */
#define BBMPC_TRACE_ELITES  4   /* int32 [A,k] (CEM), [A] best index (RandomSearch/PSO) */
#define BBMPC_TRACE_SAMPLES 5   /* [N,A,H,U] action sequences that were rolled out */
#define BBMPC_TRACE_CMA_B   6   /* CMA-ES [G,n,n] eigenvectors B after the iteration (cma_es.py:195-198,204)   */
#define BBMPC_TRACE_CMA_C   7   /* CMA-ES [G,n,n] covariance C after the iteration (cma_es.py:183-190,202)     */
#define BBMPC_TRACE_CMA_SVD_STATS 9 /* CMA-ES int32 [G,16]: the iteration's eigen-decomposition, for search dimensions 32 < n <= 512.
                                     * [0..14] column pairs the Jacobi rotated in sweep s (all zero when the direct solver's result
                                     * was taken).  [15]: with the direct solver (128 < n <= 320) 1 = it refused the instance and the
                                     * Jacobi ran for it; on the Jacobi-only paths 1 = sweep 0 rotated something.  n <= 32 (one
                                     * workgroup factorises, falls back and finishes in one kernel) records nothing: all zero. */
#define BBMPC_TRACE_CMA_D   8   /* CMA-ES [G,n]   diag(D) = sqrt(eigenvalues) after the iteration (:197,205)   */
#define BBMPC_TRACE_TOPK_PASSES 10 /* CEM int32 [A]: radix passes the iteration's elite selection took (csrc/topk.hpp); the persistent pendulum
                                     * kernel and the per-iteration refit kernels record it, every other path leaves 0.  Bit 8
                                     * (0x100) is set when the persistent kernel's all-wave route listed the winners; that
                                     * route never runs while the sorted elites are traced, so the bit shows only under the
                                     * test hook BBMPC_TRACE_SELECT_ONLY=1 (read when the handle is created), which leaves
                                     * BBMPC_TRACE_ELITES of that kernel empty */

typedef struct bbmpc_handle_s* bbmpc_handle;

/* Mirrors the constructor kwargs of OptimizerBase + the six optimizers
 * (optimizer_base.py:6-50; cem.py:7-10; pi2.py:9-11; random_search.py:7-8;
 *  pso.py:7-11; cma_es.py:7-10; spsa.py:7-12). */
typedef struct bbmpc_config {
    int32_t abi_version;        /* BBMPC_ABI_VERSION */
    int32_t optimizer;          /* BBMPC_OPT_* */
    int32_t dynamics;           /* BBMPC_DYN_* */
    int32_t reward;             /* BBMPC_REW_* */
    int32_t population_size;    /* N; above 32768 it must divide into <= 64 equal shards of <= 32768 (played in turn on the one GPU) */
    int32_t num_agents;         /* A  (agents owned by THIS handle / GPU) */
    int32_t planning_horizon;   /* H */
    int32_t dim_u;              /* U = env_action_space.shape[0] */
    int32_t dim_s;              /* S = env_observation_space.shape[0] */
    int32_t max_iterations;     /* ignored by RandomSearch */
    int32_t num_elite;          /* CEM, CMA-ES */
    int32_t agent_offset;       /* global id of local agent 0 (agent sharding; RNG is keyed by global id) */
    int32_t num_agents_global;  /* total agents across all shards (>= num_agents) */
    int32_t device;             /* HIP device ordinal, -1 = current */
    uint32_t quirks;            /* BBMPC_FIX_* / mode bits */
    uint32_t reserved0;
    uint64_t seed;              /* engine RNG seed (Philox key) */
    float alpha;                /* CEM smoothing (cem.py:10) */
    float lamda;                /* PI2 temperature (pi2.py:11) */
    float pso_c1, pso_c2, pso_w, pso_v0_fraction;           /* pso.py:9-11 */
    float spsa_alpha, spsa_gamma, spsa_a, spsa_c;           /* spsa.py:9-12 */
    float cma_alpha_cov, cma_h_sigma;                       /* cma_es.py:10 */
    const float* action_low;    /* [U] env_action_space.low  */
    const float* action_high;   /* [U] env_action_space.high */
    /* population sharding for num_agents < n_gpus (all six optimizers): this handle rolls out particles
     * [population_offset, population_offset + population_size) of a population of population_global particles that
     * every rank shares for the SAME agents; per iteration the ranks exchange (min cost, sum of weights, weighted
     * sums [H*U]) per agent (PI2, pi2.py:80-87) or their local top-k with the sample rows (CEM, cem.py:97-112) over the
     * handle's communicator (bbmpc_comm_init) and merge them in rank order, so every rank refits the same distribution.
     * 0 / 0 = not sharded. */
    int32_t population_offset;
    int32_t population_global;
} bbmpc_config;

/* ---- library ------------------------------------------------------------ */
int         bbmpc_abi_version(void);
const char* bbmpc_last_error(void);
/* number of usable gfx950 devices (0 when none; never fails) */
int         bbmpc_device_count(void);

/* ---- lifecycle ---------------------------------------------------------- */
/* Stands in for MPCPolicy.__init__ / Optimizer.__init__ + set_trajectory_evaluator
 * (policies/mpc_policy.py:58-122; optimizer_base.py:105-115). */
int bbmpc_create(const bbmpc_config* cfg, bbmpc_handle* out);
int bbmpc_destroy(bbmpc_handle h);
/* Launch on a caller-provided hipStream_t; NULL = the handle's own (non-blocking) stream.  Note that the legacy
 * default stream's handle IS NULL (PyTorch's current stream, unless the caller entered a side stream): use
 * bbmpc_set_stream_default to launch there -- or, better, run the control loop on a side stream. */
int bbmpc_set_stream(bbmpc_handle h, void* hip_stream);
int bbmpc_set_stream_default(bbmpc_handle h);   /* the legacy default (NULL) stream */

/* DeterministicMLP weights + SystemDynamicsHandler normalisation stats
 * (deterministic_mlp.py:5-25 Dense kernels [in,out] row-major, biases [out];
 *  system_dynamics_handler.py:84-95 six stats vectors).
 * dims has n_layers+1 entries, dims[0] = S+U, dims[n_layers] = S.
 * stats = {mean_states[S], std_states[S], mean_actions[U], std_actions[U],
 *          mean_targets[S], std_targets[S]} or NULL when is_normalized == 0. */
int bbmpc_set_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* activations,
                  const float* const* weights, const float* const* biases,
                  int32_t is_normalized, const float* const* stats);

/* Learned reward model for a handle created with BBMPC_DYN_MLP + BBMPC_REW_MLP: a Dense stack r(s_t, a_t, s_{t+1}) fitted
 * next to the dynamics (the reference takes any callable as reward_function, trajectory_evaluators/deterministic.py:13-18;
 * a network is one).  Layouts as bbmpc_set_mlp: Dense kernels [in, out] row-major, biases [out], dims has n_layers + 1
 * entries, dims[n_layers] == 1, any BBMPC_ACT_* code per layer.  input_mask picks the network's inputs: bit 0 = s_t,
 * bit 1 = a_t, bit 2 = s_{t+1}, at least one; the selected blocks are concatenated in that order and dims[0] is their total
 * width D.  stats = {mean_in[D], std_in[D], mean_r[1], std_r[1]} or NULL when is_normalized == 0: the input is normalised
 * as bbmpc_process_input normalises, x = (x - mean_in) / (std_in + 1e-7), and the reward is y * std_r + mean_r.
 * The handle is routed exactly as a BBMPC_DYN_MLP handle with a HIP-source BBMPC_REW_USER reward: the MFMA rollout records
 * the state after every step and a second MFMA kernel scores the trajectory -- sum over t in ascending order, NaN -> -1e6
 * per trajectory, added to -(bound penalty); a_t is the feasible (clipped) action where the optimizer clips.  Control steps
 * of all six optimizers, bbmpc_evaluate[_dev], bbmpc_evaluate_next_reward, the record's reward, bbmpc_predict_trajectories,
 * bbmpc_rollout_episode, trace / keep_plan / elite carry / sampling correlation and agent and population shards work; there
 * are no resident, fused or graph-replayed forms, BBMPC_USER_STEPWISE is ignored and BBMPC_FIX_Q1_REWARD_ARG_ORDER does not
 * apply (the network always sees (s_t, a_t, s_{t+1})).  Equal calls give equal bits, whatever the number of agents.
 * Calling it again replaces the network.  Refused before anything is allocated -- BBMPC_E_UNSUPPORTED: n_layers > 8, a
 * hidden width > 512, D > 192; BBMPC_E_INVALID: NULL pointers, n_layers < 1, a width < 1, an unknown activation,
 * input_mask outside [1, 7], dims[0] != D, dims[n_layers] != 1, is_normalized without stats; BBMPC_E_STATE: not a
 * BBMPC_REW_MLP handle.  Computing before the network is set fails with BBMPC_E_STATE.  BBMPC_E_UNSUPPORTED as well:
 * bbmpc_create with BBMPC_REW_MLP beside analytic or user dynamics, bbmpc_set_inverse_transform_source and
 * bbmpc_set_particles (num_particles > 0) on such a handle. */
int bbmpc_set_reward_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* activations,
                         const float* const* weights, const float* const* biases, int32_t input_mask,
                         int32_t is_normalized, const float* const* stats);

/* Learned terminal value for a BBMPC_DYN_MLP handle with any reward kind (built-in, HIP-source BBMPC_REW_USER, BBMPC_REW_MLP):
 * a Dense stack V(s) over the state alone that closes every rollout of a plan,
 *     R'[n, a] = R[n, a] + terminal_weight * V(s_H[n, a]),
 * where R is what the handle computes without it (the step sum, NaN -> -1e6, minus the bound penalty) and s_H the state
 * the rollout reached after its last step (after the clipped actions where the optimizer clips).  If terminal_weight * V
 * is NaN the candidate scores -1e6.  Layouts as bbmpc_set_reward_mlp with a state-only input: dims[0] == dim_s,
 * dims[n_layers] == 1, stats = {mean_in[dim_s], std_in[dim_s], mean_v[1], std_v[1]} or NULL when is_normalized == 0;
 * V = y * std_v + mean_v on x = (s - mean_in) / (std_in + 1e-7).  While a network is installed, bbmpc_evaluate[_dev] and
 * the control steps of all six optimizers (agent and population shards included) run what they ran before with the
 * trajectory recorded, then one more kernel adds the terminal term: one launch sequence per iteration, no graph-replayed
 * form.  The control step's record, bbmpc_predict_next_state, bbmpc_evaluate_next_reward and bbmpc_predict_trajectories
 * are unchanged: the term belongs to a plan, not to a step.  Calling it again replaces the network and the weight;
 * n_layers == 0 (every other argument is then ignored) removes it and restores the handle's previous routing and outputs
 * bit for bit.  Refused before anything is allocated, the handle stays as it was -- BBMPC_E_UNSUPPORTED: n_layers > 8, a
 * hidden width > 512, analytic or BBMPC_DYN_USER dynamics, a callback plug-in, an inverse target transform, particles on
 * (and, the other way round, bbmpc_set_inverse_transform_source, a callback and bbmpc_set_particles (num_particles > 0)
 * on a handle that has a value network); BBMPC_E_INVALID: NULL pointers, n_layers < 0, a width < 1, dims[0] != dim_s,
 * dims[n_layers] != 1, an unknown activation, is_normalized without stats, a non-finite terminal_weight. */
int bbmpc_set_terminal_value_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* activations,
                                 const float* const* weights, const float* const* biases, int32_t is_normalized,
                                 const float* const* stats, float terminal_weight);

/* V on `batch` rows of states [batch][dim_s] -> values [batch]: the installed network alone, without terminal_weight and
 * without a NaN rule.  BBMPC_E_STATE without a network.  The _dev form takes device pointers and is ordered on the
 * handle's stream. */
int bbmpc_evaluate_terminal_value(bbmpc_handle h, const float* states, int32_t batch, float* values);
int bbmpc_evaluate_terminal_value_dev(bbmpc_handle h, const float* d_states, int32_t batch, float* d_values);

/* Discounted, termination-aware returns of a learned-model handle (BBMPC_DYN_MLP with a built-in reward or BBMPC_REW_MLP;
 * DESIGN.md section 8q).  state_lo / state_hi are each NULL or dim_s floats (-inf / +inf: unbounded in that direction).
 * Per candidate, with s_0 the agent's state, s_1 .. s_H the model's states, a_t the clipped actions, r_t the step rewards:
 *     outside(s) = any i: s[i] < state_lo[i] or s[i] > state_hi[i]        (false on NaN: a NaN state does not terminate)
 *     g = 1; alive = true; R = 0; T = 0
 *     for t = 0 .. H-1:   R += g * r_t
 *                         if outside(s_{t+1}):  R += g * terminal_reward; alive = false; T = t + 1; stop
 *                         g *= discount
 *     if isnan(R): R = -1e6;   R += -(bound penalty)
 *     if alive and a value network is installed:  R += g * terminal_weight * V(s_H), a NaN term -> R = -1e6
 * The step that reaches a terminal state counts; nothing behind it is read into the score (a NaN there does not reach R).
 * While shaping is on, bbmpc_evaluate[_dev] and the control steps of all six optimizers (agent and population shards
 * included) record the trajectory and end in one more kernel that walks it: one launch sequence per iteration, no
 * graph-replayed form.  The control step's record, bbmpc_predict_next_state, bbmpc_evaluate_next_reward,
 * bbmpc_predict_trajectories and bbmpc_rollout_episode are unchanged.  discount == 1 with both bounds NULL switches shaping
 * off and restores the handle's previous routing and scores bit for bit.  Refused before anything is allocated, the handle
 * stays as it was -- BBMPC_E_UNSUPPORTED: analytic or BBMPC_DYN_USER dynamics, a BBMPC_REW_USER reward (HIP source or
 * callback), an inverse target transform, particles on, gradient refinement on (and, the other way round,
 * bbmpc_set_inverse_transform_source, bbmpc_set_particles (num_particles > 0) and bbmpc_set_grad_refine (steps > 0) on a
 * handle with shaping on; bbmpc_plan_gradient[_dev] and bbmpc_refine_plans[_dev] are refused while it is on, their return
 * is not the shaped one); BBMPC_E_INVALID: a discount outside (0, 1] or not finite, a NaN bound, state_lo[i] >
 * state_hi[i], a non-finite terminal_reward. */
int bbmpc_set_return_shaping(bbmpc_handle h, float discount, const float* state_lo, const float* state_hi, float terminal_reward);

/* T of the most recent rollout (bbmpc_evaluate, or the last iteration of a control step): out [num_agents][n_pop] int32, the
 * first terminal step in 1 .. H or 0 when the candidate never left the box; n = num_agents * n_pop.  BBMPC_E_STATE while
 * shaping is off or before anything was rolled out. */
int bbmpc_get_termination_steps(bbmpc_handle h, int32_t* out, int32_t n);

/* Plan gradients: the derivative of the model return with respect to every action of a plan, through the learned dynamics
 * (BBMPC_DYN_MLP, bbmpc_set_mlp), the learned reward (BBMPC_REW_MLP, bbmpc_set_reward_mlp, any input_mask) and, when one is
 * installed, the learned terminal value.  For row b, s_0 = states[b] and a_0 .. a_{horizon-1} = seq[b]:
 *     s_{t+1} = the learned model's noise-free step (bbmpc_predict_trajectories' rule), r_t = RewardMLP(s_t, a_t, s_{t+1}),
 *     R[b] = sum over t ascending of r_t + terminal_weight * V(s_horizon)        (the last term only with a value network)
 *     grad_out[b, t, u] = dR[b] / da_t[u],      returns_out[b] = R[b]   (returns_out may be NULL)
 * by reverse accumulation in one kernel launch.  Actions are used as given: no clip, no bound penalty, no NaN rule (NaN
 * propagates).  At a kink of relu, relu6, leaky_relu or hard_sigmoid the derivative is that of the branch the forward's
 * comparison takes.  A rows call like bbmpc_predict_trajectories: the handle's optimizer, particles, colored noise, elite
 * carry and policy prior play no part, and nothing of the handle changes but a workspace of its own that grows on demand.
 * Deterministic: two calls give equal bits, and a batch split at a multiple of 16 rows equals the whole bit for bit.
 * Refused before anything is allocated, the handle stays as it was -- BBMPC_E_UNSUPPORTED: dynamics other than
 * BBMPC_DYN_MLP, a reward kind other than BBMPC_REW_MLP, a model ensemble or log-variance heads, an inverse target
 * transform, a callback plug-in, networks whose activation tiles do not fit one CU's LDS, a workspace of 2^31 elements or
 * more (split the batch); BBMPC_E_STATE: bbmpc_set_mlp or bbmpc_set_reward_mlp not called yet; BBMPC_E_INVALID: NULL
 * states / seq / grad_out, batch < 1, horizon outside [1, 4096].  The _dev form takes device pointers and is ordered on
 * the handle's stream. */
int bbmpc_plan_gradient(bbmpc_handle h, const float* states, const float* seq, int32_t batch, int32_t horizon,
                        float* returns_out, float* grad_out);
int bbmpc_plan_gradient_dev(bbmpc_handle h, const float* d_states, const float* d_seq, int32_t batch, int32_t horizon,
                            float* d_returns_out, float* d_grad_out);

/* Plan refinement on the device: projected gradient ascent on the model return of bbmpc_plan_gradient,
 * the whole loop on the handle's stream.  states [batch][dim_s]; seq [batch][horizon][dim_u] is refined IN PLACE.  Every step:
 * gradient, then method 0 (Adam, beta 0.9 / 0.999, epsilon 1e-8, on the ascent direction) or 1 (plain ascent), a non-finite
 * step element counting as 0, x <- clip(x + lr * step, action_low[u], action_high[u]) with the handle's bounds; moments start
 * at zero in every call.  keep_best = 1: steps + 1 gradient calls, seq receives per row the best plan by model return, the
 * input included (a NaN return never replaces anything), returns_out [batch] (may be NULL) its return; steps = 0 returns the
 * input and its return.  keep_best = 0: steps gradient calls, seq receives the last iterate, and returns_out, when not NULL,
 * costs one more call that scores it.  Refusals: those of bbmpc_plan_gradient, checked before anything is allocated, and
 * BBMPC_E_INVALID for steps outside [0, 64], lr not finite or not positive, method outside {0, 1}, keep_best outside
 * {0, 1}.  The _dev form takes device pointers, is ordered on the handle's stream and does not wait for it. */
int bbmpc_refine_plans(bbmpc_handle h, const float* states, float* seq, int32_t batch, int32_t horizon, int32_t steps, float lr,
                       int32_t method, int32_t keep_best, float* returns_out);
int bbmpc_refine_plans_dev(bbmpc_handle h, const float* d_states, float* d_seq, int32_t batch, int32_t horizon, int32_t steps,
                           float lr, int32_t method, int32_t keep_best, float* d_returns_out);
/* Gradient steps on CEM's candidates (GradCEM).  In every CEM iteration, after the draw, the policy-prior
 * rollouts and the elite injection, the last `candidates` columns of every agent (0: all population_size) take `steps`
 * steps of bbmpc_refine_plans_dev(keep_best = 0, returns_out = NULL) from that agent's current state; the rollout then scores
 * the buffer as it does otherwise, and the trace's samples are the refined candidates.  While it is on, control steps run one
 * launch sequence per iteration (no resident, fused or graph-replayed form).  steps = 0 switches it off.
 * BBMPC_E_UNSUPPORTED: an optimizer other than CEM, a handle bbmpc_plan_gradient would refuse, particles, a sharded
 * population (particles, a model ensemble and log-variance heads are refused by their own setters while it is on).
 * BBMPC_E_INVALID: steps outside [0, 64], lr not finite or not positive, method outside {0, 1}, candidates outside
 * [0, population_size].  Networks not yet installed: BBMPC_E_STATE at the control step.  A refused call leaves the handle as
 * it was.  bbmpc_reset keeps the setting. */
int bbmpc_set_grad_refine(bbmpc_handle h, int32_t steps, float lr, int32_t method, int32_t candidates);
/* The setting; steps = 0 (and zeros) while it is off. */
int bbmpc_get_grad_refine(bbmpc_handle h, int32_t* steps, float* lr, int32_t* method, int32_t* candidates);

/* User-supplied plug-ins.  The reference takes ANY callable as reward_function / dynamics_function
 * (trajectory_evaluators/deterministic.py:13-18; called at :65-66 as reward(current_state, actions, next_state) and at
 * :99-100 as dynamics(x[B,S+U], train=False) -> delta[B,S]).  A Python callable cannot run inside a kernel; the
 * counterpart is HIP source, compiled at run time (hiprtc, gfx950), that defines per row
 *     __device__ float bbmpc_user_reward(const float* cur, const float* act, const float* nxt, int S, int U);
 *     __device__ void  bbmpc_user_dynamics(const float* x, float* delta, int S, int U);     (x = [state | action])
 * for a handle created with BBMPC_REW_USER / BBMPC_DYN_USER (user dynamics are a true model: next = state + delta,
 * utils/transforms.py:34).  Any combination with the built-in plug-ins works; evaluation then runs step by step
 * (one batched dynamics and one batched reward launch per planning step, as the reference's own graph does) instead
 * of through the built-in pairs' fused kernels -- unless the dynamics is analytic (user or PendulumTrueModel): then the
 * engine compiles ONE fused lane-per-trajectory rollout kernel with the user function(s) inlined.  Compile errors come back as BBMPC_E_INVALID with the compiler log in
 * bbmpc_last_error().  bbmpc_check_user_source only compiles (needs no GPU): kind 1 = reward, 2 = dynamics. */
int bbmpc_set_reward_source(bbmpc_handle h, const char* hip_source);
int bbmpc_set_dynamics_source(bbmpc_handle h, const char* hip_source);
int bbmpc_check_user_source(int32_t kind, const char* hip_source, int32_t dim_s, int32_t dim_u);
/* The same two plug-ins as HOST callbacks that work on DEVICE memory -- for callers whose functions are written in a
 * GPU array framework (the reference's users pass TensorFlow callables, deterministic.py:13-18; the Python layer wraps
 * PyTorch callables this way).  The engine calls back once per planning step with row batches that
 * live in its own HBM buffers; the callback enqueues its work on `hip_stream` (the handle's launch stream) and
 * returns without synchronising -- nothing is copied to the host, nothing runs on the CPU but the enqueueing.
 *   reward:   d_cur [batch,S], d_actions [batch,U], d_next [batch,S]  ->  d_out [batch]     (the reference's CALL order)
 *   dynamics: d_cur [batch,S], d_actions [batch,U], d_next = NULL     ->  d_out [batch,S] = the ABSOLUTE next states, i.e.
 *             process_output(state, f(process_input(state, action))) of dynamics_handlers/system_dynamics_handler.py:97-161
 * A non-zero return aborts the control step with BBMPC_E_INVALID.  A handle with a callback evaluates step by step
 * (2 * H + 2 launches plus the callback's own); setting a callback replaces HIP source of the same kind and vice versa.
 * fn == NULL clears it. */
typedef int32_t (*bbmpc_rows_callback)(void* user, const float* d_cur, const float* d_actions, const float* d_next,
                                       int32_t batch, float* d_out, void* hip_stream);
int bbmpc_set_reward_callback(bbmpc_handle h, bbmpc_rows_callback fn, void* user);
int bbmpc_set_dynamics_callback(bbmpc_handle h, bbmpc_rows_callback fn, void* user);
/* Compile-only check of the FUSED rollout kernel the engine builds for analytic models (one lane per trajectory, the
 * user function(s) inlined next to the built-in PendulumTrueModel / rewards): dynamics / reward = BBMPC_DYN_* /
 * BBMPC_REW_* kinds, sources NULL for built-ins.  Needs no GPU. */
int bbmpc_check_user_rollout(int32_t dynamics, int32_t reward, const char* dynamics_source, const char* reward_source,
                             int32_t dim_s, int32_t dim_u);
/* Runtime parameters of HIP-source plug-ins: goals, setpoints, reference trajectories or estimated plant constants that
 * change between control steps without a recompile.  A source set with bbmpc_set_*_source_params(h, src, P) defines
 * the parameterised entry point instead of the classic one:
 *     __device__ float bbmpc_user_reward_params(const float* cur, const float* act, const float* nxt, int S, int U,
 *                                               const float* params, int t);
 *     __device__ void  bbmpc_user_dynamics_params(const float* x, float* delta, int S, int U, const float* params, int t);
 * `params` is the P-float row of the agent that owns the row being scored (read only); t is the planning step inside
 * the horizon, 0 for the one-step calls (the control step's next state and reward, bbmpc_predict_next_state,
 * bbmpc_evaluate_next_reward, bbmpc_step_dev).  Every kernel that calls the function gets the row: the fused
 * analytic rollout, the step-wise evaluator, the learned model's trajectory scorer and its transform rollout.  The
 * program is compiled with BBMPC_REW_NPARAMS / BBMPC_DYN_NPARAMS = P (a source without parameters compiles exactly
 * as before).  Limits: 1 <= P <= BBMPC_MAX_USER_PARAMS floats per agent (BBMPC_E_INVALID below, BBMPC_E_UNSUPPORTED
 * above).
 * bbmpc_set_user_params(h, kind, data, count): kind 1 = reward, 2 = dynamics; host data of count = P floats (shared by
 * every agent) or num_agents * P (one row per LOCAL agent, agent-major).  It only uploads, on the handle's stream
 * behind the work already queued, and returns once the copy is done.  BBMPC_E_STATE when the handle's function of that
 * kind has no parameters, BBMPC_E_INVALID for any other count.  Computing with a parameterised function whose
 * parameters were never set fails with BBMPC_E_STATE; a one-step call on B rows with per-agent parameters needs B to be
 * a multiple of num_agents (B / A consecutive rows per agent) and fails with BBMPC_E_INVALID otherwise.
 * bbmpc_compile_stats: the number of hiprtc compilations this handle has run (sources, transforms and the fused
 * rollouts it builds lazily) -- a parameter update never adds one.
 * bbmpc_check_user_params compiles (no GPU) every program a parameterised reward and/or dynamics takes part in: the
 * row kernels (and the trajectory scorer), the fused rollouts with each built-in and user partner, and the learned
 * model's transform rollout with the reward inlined; a missing partner source is a classic stub.  A NULL source skips
 * that side. */
#define BBMPC_MAX_USER_PARAMS 4096
int bbmpc_set_reward_source_params(bbmpc_handle h, const char* hip_source, int32_t num_params);
int bbmpc_set_dynamics_source_params(bbmpc_handle h, const char* hip_source, int32_t num_params);
int bbmpc_set_user_params(bbmpc_handle h, int32_t kind, const float* data, int64_t count);
int bbmpc_compile_stats(bbmpc_handle h, int64_t* compiles);
int bbmpc_check_user_params(const char* reward_source, int32_t reward_params, const char* dynamics_source,
                            int32_t dynamics_params, int32_t dim_s, int32_t dim_u);
/* Target transforms: SystemDynamicsHandler's transform_targets_func / inverse_transform_targets_func (reference
 * dynamics_handlers/system_dynamics_handler.py:15-17, 128-161, 314) as HIP source (hiprtc, gfx950) defining per row
 *     __device__ void bbmpc_user_inverse_transform_targets(const float* cur, const float* dev, float* next, int S);
 *     __device__ void bbmpc_user_transform_targets(const float* cur, const float* next, float* target, int S);
 * `dev` is the de-normalised model output (mean_t + raw * (std_t + 1e-7) for a normalised learned model, the raw
 * output otherwise).  bbmpc_set_inverse_transform_source puts it in place of next = dev + state everywhere on a
 * BBMPC_DYN_MLP or BBMPC_DYN_USER handle: rollouts (learned model: one MFMA kernel compiled with the transform and a
 * user reward inlined; BBMPC_USER_STEPWISE=1: the step-wise evaluator), predict_next_state and the control step's next
 * state.  NULL / "" clears it.  bbmpc_set_transform_source sets the forward transform, which only
 * bbmpc_transform_rows uses (training targets).  bbmpc_transform_rows: kind 3 -> out = inverse(a = cur, b = dev),
 * kind 4 -> out = forward(a = cur, b = next); host arrays [batch, S].  bbmpc_check_user_source takes kinds 3 / 4;
 * bbmpc_check_xform_rollout compiles the fused learned-model rollout (reward: BBMPC_REW_*, reward_source for
 * BBMPC_REW_USER).  Neither check needs a GPU. */
int bbmpc_set_inverse_transform_source(bbmpc_handle h, const char* hip_source);
int bbmpc_set_transform_source(bbmpc_handle h, const char* hip_source);
int bbmpc_transform_rows(bbmpc_handle h, int32_t kind, const float* a, const float* b, int32_t batch, float* out);
int bbmpc_check_xform_rollout(int32_t reward, const char* transform_source, const char* reward_source, int32_t dim_s,
                              int32_t dim_u);
/* DeterministicMLP.__call__(x[B, S+U], train) -> [B, S]: the raw Dense stack on already-processed inputs
 * (dynamics_functions/deterministic_mlp.py:27-51), no normalisation, no residual. */
int bbmpc_mlp_forward(bbmpc_handle h, const float* x, int32_t batch, float* out);

/* SystemDynamicsHandler.process_input(states[B,S], actions[B,U]) -> [B,S+U] and .process_output(states[B,S],
 * raw_output[B,S]) -> next_states[B,S] as stand-alone calls (dynamics_handlers/system_dynamics_handler.py:97-161 +
 * utils/transforms.py:20-34).  stats = the six statistics vectors in bbmpc_set_mlp's order for a normalised learned
 * model, NULL for a true model / un-normalised handler (plain concat; next = raw + state).  Inside rollouts the same
 * arithmetic is fused into the kernels (prologue / epilogue). */
int bbmpc_process_input(bbmpc_handle h, const float* states, const float* actions, int32_t batch,
                        const float* const* stats, float* out);
int bbmpc_process_output(bbmpc_handle h, const float* states, const float* raw_output, int32_t batch,
                         const float* const* stats, float* out);

/* Optimizer.reset()  (cem.py:138-149, pi2.py:98-105, pso.py:143-160, cma_es.py:215-227, spsa.py:119-127) */
int bbmpc_reset(bbmpc_handle h);

/* ---- hot path ----------------------------------------------------------- */
/* OptimizerBase.__call__(current_state, time_step, add_exploration_noise)
 * -> (action[A,U], next_state[A,S], reward[A])      optimizer_base.py:55-95
 * Host buffers in, host buffers out, synchronous.  On the analytic path with up to 64 agents the control step's kernel
 * stays resident on the GPU for BBMPC_LINGER_US (default 200) after the call returns and serves the next bbmpc_optimize
 * without a launch; any other entry point of the handle stops it first, and a device-wide synchronisation by the
 * caller waits at most that long.  Results do not depend on it (BBMPC_LINGER_US=0: one launch per call). */
int bbmpc_optimize(bbmpc_handle h, const float* state, int32_t time_step, int32_t add_exploration_noise,
                   float* action, float* next_state, float* reward);
/* How the host-in / host-out calls (bbmpc_optimize, bbmpc_optimize_gather) of this handle were served so far: by the
 * resident kernel of the previous call (request mailbox, no launch) or by launching.  Either pointer may be NULL.
 * No counterpart in the reference (its act() is one TF graph call per control step, policies/mpc_policy.py:160-164);
 * exists so that a benchmark can say which of the two paths its number was measured on. */
int bbmpc_call_stats(bbmpc_handle h, int64_t* served_resident, int64_t* launched);
/* ... and how many of the launched ones were replays of a captured hipGraph (the steady-state control step of the
 * learned-model PI2 / CEM path: same launches, same arguments every call).  No counterpart in the reference. */
int bbmpc_graph_stats(bbmpc_handle h, int64_t* replayed);
/* (A capture or instantiation that fails switches the replay off for the handle and the calls go on as plain launches;
 * BBMPC_TRACE_GRAPH=1 in the environment reports it on stderr.) */
/* The GPU the handle lives on: bbmpc_config.device, or the caller's current HIP device at bbmpc_create when that was < 0.
 * Callers that alias the handle's HBM buffers or stream in another framework must do so on THIS device. */
int bbmpc_handle_device(bbmpc_handle h, int32_t* device);

/* Same with device pointers; record is [A, U+S+1] = (action | next_state | reward) per agent.
 * d_next_state (optional, may be NULL) additionally receives the predicted next state as a contiguous
 * [A,S] tensor, so a closed-loop caller can feed it straight back as the next d_state. */
int bbmpc_optimize_dev(bbmpc_handle h, const float* d_state, int32_t time_step, int32_t add_exploration_noise,
                       float* d_record, float* d_next_state);

/* DeterministicTrajectoryEvaluator.__call__(current_states[A,S], action_sequences[n_pop,A,H,U], t)
 * -> rewards[n_pop,A]                 trajectory_evaluators/deterministic.py:26-77 */
int bbmpc_evaluate(bbmpc_handle h, const float* state, const float* action_sequences, int32_t n_pop,
                   float* rewards);
int bbmpc_evaluate_dev(bbmpc_handle h, const float* d_state, const float* d_action_sequences, int32_t n_pop,
                       float* d_rewards);

/* Particle trajectory evaluator: the "different trajectory evaluators to propagate uncertainties" the reference's README
 * leaves open (its EvaluatorBase / set_trajectory_evaluator layout was made for them).  Every candidate is rolled out
 * num_particles times through the handle's ONE model with additive Gaussian process noise, for agent a, candidate n,
 * particle p:   s_0 = state[a];   nxt = predict_next_state(s_t, a_t) + sigma (.) eps[a, p, t, :];
 *               R += reward(s_t, a_t, nxt) (the reference's call order, quirk Q1 as configured);   s_{t+1} = nxt
 * r[n,p,a] = R (NaN -> -1e6 per particle);  mean = (sum_p r) / P and var = (sum_p (r - mean)^2) / P in index order, fp32;
 * score[n,a] = mean - risk_kappa * sqrt(var)  (risk_kappa == 0: the mean).  eps does not depend on the candidate
 * (common random numbers); it is drawn per optimizer iteration from stream BBMPC_NOISE_PROCESS -- Philox counter
 * (p, ga * Qp + (j >> 2), control_step, (11 << 16) | iter), ga the global agent id, j = t * S + s, Qp = ceil(H * S / 4),
 * element j from word j & 3, Box-Muller on word pairs as BBMPC_NOISE_NORMAL -- or injected (bbmpc_inject_noise).
 * With particles on, every optimizer scores its candidates this way (bound penalties are subtracted from the score),
 * bbmpc_evaluate[_dev] returns the scores (iter = 0, the handle's current control step: equal calls give equal bits) and
 * control steps take one launch sequence per iteration, as with bbmpc_set_trace.  The control step's record stays the
 * noise-free one-step prediction.  On the analytic pendulum the noise lands on (cos, sin, thdot), so the rollouts use the
 * op-for-op model step whatever BBMPC_STRICT_MATH says.  num_particles = 0 switches back to the deterministic paths, bit
 * for bit.  BBMPC_E_INVALID: num_particles outside [0, 64], sigma NULL / negative / not finite, risk_kappa not finite.
 * BBMPC_E_UNSUPPORTED: HIP-source or callback reward / dynamics, an inverse target transform, a sharded population,
 * population_size * num_particles > 32768.
 * bbmpc_evaluate_particles: scores [n_pop, A] and, when `returns` is not NULL, the per-particle returns [n_pop, P, A]
 * (BBMPC_E_STATE with particles off).  The host variant is synchronous; _dev enqueues on the handle's stream. */
int bbmpc_set_particles(bbmpc_handle h, int32_t num_particles, const float* sigma, float risk_kappa);
int bbmpc_evaluate_particles(bbmpc_handle h, const float* state, const float* action_sequences, int32_t n_pop,
                             float* scores, float* returns);
int bbmpc_evaluate_particles_dev(bbmpc_handle h, const float* d_state, const float* d_action_sequences, int32_t n_pop,
                                 float* d_scores, float* d_returns);

/* How the particle evaluator reduces the P returns of a candidate to its score.  BBMPC_RISK_MEAN_STD (the default):
 * mean - risk_kappa * std as above; tail_count must be 0.  BBMPC_RISK_CVAR: the conditional value at risk of the lower
 * tail, the mean of the tail_count worst returns (1 <= tail_count <= num_particles; tail_count = 1 is the worst case over
 * the particles) -- with the stable rank  rank[p] = #{q : r[q] < r[p]} + #{q < p : r[q] == r[p]}  (equal returns are
 * ordered by particle index, every comparison exact),
 *     score[n,a] = (sum of r[n,p,a] over the p with rank[p] < tail_count, in particle index order) / (float)tail_count
 * in fp32, so the selection is exact given the returns and tail_count = num_particles gives the bits of the risk_kappa = 0
 * mean.  risk_kappa is ignored under CVaR.  Everything else of bbmpc_set_particles is unchanged: the returns (NaN -> -1e6 per
 * particle, so no NaN is ranked), the noise, the bound penalties subtracted from the score, the feasible samples written
 * back; all six optimizers then plan on the CVaR score, and bbmpc_evaluate[_particles] returns it.  The setting is handle
 * state: it may be made before or after bbmpc_set_particles and survives bbmpc_set_particles(0).
 * BBMPC_E_INVALID: an unknown kind, tail_count != 0 with MEAN_STD, tail_count outside [1, 64], tail_count > num_particles --
 * from whichever of bbmpc_set_particles / bbmpc_set_particle_risk comes second.  A refused call leaves the handle as it was. */
#define BBMPC_RISK_MEAN_STD 0
#define BBMPC_RISK_CVAR     1
int bbmpc_set_particle_risk(bbmpc_handle h, int32_t kind, int32_t tail_count);

/* Chance constraint of the particle evaluator: a state box [lo, hi] ([dim_S] each, -inf / +inf =
 * unbounded in that feature) that does NOT end a rollout.  The share of a candidate's particles that ever leave the box
 * becomes a penalty on its score; per agent a, candidate n, particle p, with s_1 .. s_H the noisy next states of the
 * particle recurrence above (s_0 is given and not tested):
 *     out(s)       = any i: s[i] < lo[i] or s[i] > hi[i]     (both false on NaN: a NaN state violates nothing)
 *     first[n,p,a] = the smallest t in 1 .. H with out(s_t), else 0
 *     v[n,a]       = (float)#{p : first[n,p,a] != 0} / (float)P
 *     score'[n,a]  = score[n,a] - weight * max(0, v[n,a] - max_violation)          (fp32, in this order)
 * score is what the handle computes without the constraint (mean - kappa * std or CVaR, minus the bound penalty); the
 * per-particle returns are not changed.  All six optimizers then plan on score', bbmpc_evaluate[_particles] returns it.
 * Needs BBMPC_DYN_MLP dynamics (plain, ensemble or log-variance heads), particles on, and a built-in or HIP-source reward.
 * lo == hi == NULL removes the constraint: the handle then launches and scores what it did before, bit for bit.
 * bbmpc_set_particles(h, 0, ..) removes it as well; another num_particles keeps it.  Installing or removing it
 * invalidates a captured step graph.  The record of a control step, the one-step calls, bbmpc_predict_trajectory_particles /
 * _quantiles and every deterministic path never read it.
 * BBMPC_E_INVALID: exactly one of lo / hi NULL, a NaN bound, lo[i] > hi[i], max_violation outside [0, 1) or not finite,
 * weight negative or not finite.  BBMPC_E_UNSUPPORTED: dynamics other than BBMPC_DYN_MLP, a callback reward.
 * BBMPC_E_STATE: particles are off.  With it installed, horizon * num_agents * dim_s * (candidates rounded up to 64 *
 * num_particles) must stay below 2^31 per rollout (BBMPC_E_UNSUPPORTED from the computing call).  A refused call leaves the
 * handle as it was.
 * bbmpc_get_constraint_violations: v of the handle's most recent particle rollout as prob_out [n_pop, A] and, when
 * first_step_out is not NULL, first as [n_pop, P, A].  Synchronous.  BBMPC_E_STATE: no constraint installed, or nothing
 * rolled out since it was.  BBMPC_E_INVALID: prob_out NULL, n_pop different from that rollout's. */
int bbmpc_set_chance_constraint(bbmpc_handle h, const float* lo, const float* hi, float max_violation, float weight);
int bbmpc_get_constraint_violations(bbmpc_handle h, int32_t n_pop, float* prob_out, int32_t* first_step_out);

/* Model ensemble with trajectory sampling for the particle evaluator (PETS, TS-infinity): num_members networks of the shape,
 * activations and six normalisation statistics of the model that bbmpc_set_mlp installed, e.g. fitted on bootstrap
 * resamples of the training rows.  weights / biases: num_members x n_layers pointers, member-major (entry e * n_layers + l),
 * each in bbmpc_set_mlp's layout.  With particles on, particle p of every candidate and agent is rolled through member
 * p % num_members for the whole horizon, so member disagreement shows as spread of the per-particle returns and
 * risk_kappa > 0 penalises candidates the members disagree about.  Everything else of bbmpc_set_particles' recurrence is
 * unchanged: sigma (.) eps[a, p, t, :] on the next state (sigma = 0 leaves pure model disagreement), the reward's call
 * order, NaN -> -1e6 per particle, the noise keying and injection, the aggregate, the bound penalties; r[n, p, a] of
 * bbmpc_evaluate_particles belongs to member p % num_members.  Every deterministic path -- the control step's record,
 * bbmpc_predict_next_state, bbmpc_predict_trajectories, everything with particles off -- keeps the model of bbmpc_set_mlp,
 * and a handle without an ensemble launches what it launched before.  num_members = 0 removes the ensemble (weights and
 * biases are not read); so does a later bbmpc_set_mlp.
 * BBMPC_E_STATE: not a BBMPC_DYN_MLP handle, or bbmpc_set_mlp has not been called.  BBMPC_E_UNSUPPORTED: num_members
 * outside [0, 8].  BBMPC_E_INVALID: NULL pointers; num_particles % num_members != 0 -- from whichever of
 * bbmpc_set_particles / bbmpc_set_mlp_ensemble comes second (the members carry equal weight in the mean).  A refused call
 * leaves the handle as it was. */
int bbmpc_set_mlp_ensemble(bbmpc_handle h, int32_t num_members, const float* const* weights, const float* const* biases);

/* Probabilistic models for the particle evaluator (PETS' Gaussian heads): every model of the particle rollouts -- the model of
 * bbmpc_set_mlp, or each member of bbmpc_set_mlp_ensemble -- gets a log-variance head, a second last Dense layer on the same
 * last hidden activation h with no activation of its own, in the target space of the mean (normalised when is_normalized).
 * weights / biases: num_heads pointers to kernels [dims[n_layers - 1], dim_S] and biases [dim_S]; min_logvar / max_logvar
 * [dim_S].  With z = h W_v + b_v and softplus(x) = max(x, 0) + log(1 + exp(-|x|)):
 *     lv1 = max_logvar - softplus(max_logvar - z);   lv = min_logvar + softplus(lv1 - min_logvar)
 *     sd[f] = tstd[f] * exp(lv[f] / 2)                (tstd = std_targets + 1e-7, or 1 when not normalised)
 * and the particle recurrence of bbmpc_set_particles changes in one term:
 *     nxt = predict_next_state_member(s_t, a_t) + (sigma[f] + sd_f(s_t, a_t)) * eps[a, p, t, f]
 * on the same eps (keying, injection), reward order, NaN rule, aggregate and returns layout; sigma = 0 leaves the learned
 * noise alone.  Every deterministic path -- the record, bbmpc_predict_next_state, bbmpc_predict_trajectories, everything
 * with particles off -- keeps the mean network and launches what it launched before, as does a handle without heads.
 * Call order: bbmpc_set_mlp, optionally bbmpc_set_mlp_ensemble, then this call with num_heads = max(1, num_members): head e
 * belongs to member e, head 0 to the model when there is no ensemble.  num_heads = 0 (nothing else is read), a later
 * bbmpc_set_mlp or a later bbmpc_set_mlp_ensemble removes the heads.
 * BBMPC_E_STATE: not a BBMPC_DYN_MLP handle, or bbmpc_set_mlp has not been called.  BBMPC_E_INVALID: NULL pointers; a wrong
 * num_heads; bounds that are not finite, lie outside [-40, 40] or have min > max.  BBMPC_E_UNSUPPORTED: the doubled last
 * layer's partial sums no longer fit the kernel's LDS layout.  A refused call leaves the handle as it was. */
int bbmpc_set_mlp_logvar_head(bbmpc_handle h, int32_t num_heads, const float* const* weights, const float* const* biases,
                              const float* min_logvar, const float* max_logvar);

/* .predict_next_state(states[B,S], actions[B,U]) -> [B,S]      deterministic.py:79-103 */
int bbmpc_predict_next_state(bbmpc_handle h, const float* states, const float* actions, int32_t batch,
                             float* next_states);
/* .evaluate_next_reward(cur[B,S], next[B,S], actions[B,U]) -> [B]   deterministic.py:105-127 */
int bbmpc_evaluate_next_reward(bbmpc_handle h, const float* states, const float* next_states,
                               const float* actions, int32_t batch, float* rewards);
/* device-pointer env step used by the closed-loop harness: action rows are read with
 * `action_stride` floats between consecutive rows (so a record buffer can be passed). */
int bbmpc_step_dev(bbmpc_handle h, const float* d_states, const float* d_actions, int32_t action_stride,
                   int32_t batch, float* d_next_states, float* d_rewards);

/* Open-loop trajectory prediction: predict_next_state and evaluate_next_reward (deterministic.py:79-127) composed
 * `horizon` times from every row's own start state, all of it kept.  states [B,S], action_sequences [B,Hq,U] ->
 * states_out [B,Hq,S], rewards_out [B,Hq] (row major, row b first; either output may be NULL, not both).  With
 * s_0 = states[b], for t = 0 .. Hq-1: s_{t+1} = predict_next_state(s_t, a_t) (process_input -> model -> process_output,
 * an inverse target transform included), states_out[b,t] = s_{t+1}, rewards_out[b,t] = reward(s_t, a_t, s_{t+1}).
 * Actions are used as given (no clip, no penalty, as bbmpc_evaluate) and per-step values are returned as computed: the
 * evaluator's NaN -> -1e6 rule belongs to its sum.  Hq is independent of the handle's planning_horizon (1 <= Hq <=
 * 4096); any handle serves, evaluator-only ones included.  Built-in pendulum and learned model + built-in reward: one
 * kernel for all Hq steps; HIP-source dynamics / rewards on an analytic model: one run-time compiled kernel, built on the
 * handle's first prediction (one hiprtc run, counted by bbmpc_compile_stats; never on a handle that does not predict);
 * torch callbacks, and a learned model with an inverse target transform or a HIP-source reward, run their row kernels /
 * callbacks step by step, compiling nothing.  Runtime parameters: row b belongs to agent b / (B / A)
 * (B % A != 0 with per-agent parameters: BBMPC_E_INVALID) and the function sees t = the step inside the sequence.
 * BBMPC_E_INVALID: batch < 1, horizon outside [1, 4096], both outputs NULL; BBMPC_E_STATE: weights, sources or
 * parameters not set.  The host variant is synchronous; _dev enqueues on the handle's stream. */
int bbmpc_predict_trajectories(bbmpc_handle h, const float* states, const float* action_sequences, int32_t batch,
                               int32_t horizon, float* states_out, float* rewards_out);
int bbmpc_predict_trajectories_dev(bbmpc_handle h, const float* d_states, const float* d_action_sequences, int32_t batch,
                                   int32_t horizon, float* d_states_out, float* d_rewards_out);
/* Plan readback.  bbmpc_set_keep_plan(h, 1) makes the control steps that follow keep their solution in HBM: it routes
 * them as bbmpc_set_trace does (one launch per iteration instead of the resident / fused / graph-replayed forms, which
 * keep it in registers or LDS; same results, slower) -- off by default, and with it off nothing changes.
 * bbmpc_get_plan writes the action sequence [A,H,U] the LAST control step took its action from: the final mean (CEM, PI2,
 * SPSA, CMA-ES; before the warm-start shift), PSO's global best, RandomSearch's best particle; actions[a,0] is the action
 * that step returned without exploration noise.  BBMPC_E_STATE when the switch was not on during that step.  Roll it out
 * with bbmpc_predict_trajectories for the predicted states and rewards (OptimizerBase.plan / MPCPolicy.plan do). */
int bbmpc_set_keep_plan(bbmpc_handle h, int32_t enabled);
int bbmpc_get_plan(bbmpc_handle h, float* actions);
/* Multi-step model error: d_sum_sq[t * S + s] = sum over the B rows of (predicted[b,t,s] - observed[b,t,s])^2, device
 * arrays [B,Hq,S], the sums in float64 [Hq * S].  Two-stage reduction in a fixed order, no atomics: equal inputs give
 * equal bits.  On the handle's stream.  No counterpart in the reference (its train() reports a one-step loss only). */
int bbmpc_trajectory_sq_error_dev(bbmpc_handle h, const float* d_predicted, const float* d_observed, int32_t batch,
                                  int32_t horizon, double* d_sum_sq);
/* Trajectory distributions: the particle recurrence of bbmpc_set_particles (with the ensemble of bbmpc_set_mlp_ensemble
 * and the heads of bbmpc_set_mlp_logvar_head when they are installed) from every row's OWN start state, every state and
 * reward kept, and their per-step moments over the particles.  Needs bbmpc_set_particles on the handle: P and sigma are
 * the handle's, risk_kappa plays no part.  states [B,S], action_sequences [B,Hq,U], eps [B,P,Hq,S] standard normals or
 * NULL; for every row b and particle p, with s_0 = states[b], for t = 0 .. Hq-1:
 *     nxt = predict_next_state_member(p % E)(s_t, a[b,t]) + (sigma + sd(s_t, a[b,t])) (.) eps[b,p,t,:]
 *     particle_states[b,p,t] = nxt;  particle_rewards[b,p,t] = reward(s_t, a[b,t], nxt);  s_{t+1} = nxt
 *     mean[b,t,f] = (sum_p x[b,p,t,f]) / P;  std[b,t,f] = sqrt(sum_p (x[b,p,t,f] - mean[b,t,f])^2 / P)
 * (fp32, p in index order, as the scores of bbmpc_evaluate_particles; the same for the rewards).  Outputs: state_mean /
 * state_std [B,Hq,S], reward_mean / reward_std [B,Hq], particle_states [B,P,Hq,S], particle_rewards [B,P,Hq]; any of them
 * may be NULL, not all six.  As in bbmpc_predict_trajectories the actions are used as given, per-step values are returned as
 * computed (no clip, no penalty, no NaN -> -1e6), Hq is independent of the planning horizon (1 <= Hq <= 4096) and any
 * handle that bbmpc_set_particles accepts serves.  eps == NULL: the handle's own draws -- the BBMPC_NOISE_PROCESS stream
 * with row b in the agent word (agent_offset + b), Qp = ceil(Hq * S / 4), the handle's current control step, iteration 0:
 * at B = num_agents, Hq = planning_horizon exactly the tensor bbmpc_evaluate_particles rolls.  Equal calls give equal bits.
 * An injected BBMPC_NOISE_PROCESS tensor is not read here (its layout is the planning horizon's): pass it as eps.
 * BBMPC_E_STATE: particles off, learned model without weights; BBMPC_E_INVALID: batch < 1, horizon outside [1, 4096], all
 * outputs NULL; BBMPC_E_UNSUPPORTED: B * P * Hq * S >= 2^31, B * Hq * U >= 2^31, B * Qp >= 2^32, a network whose buffers do
 * not fit the LDS (as the particle rollouts).  The host variant is synchronous (eps a host pointer); _dev enqueues on the
 * handle's stream (eps a device pointer). */
int bbmpc_predict_trajectory_particles(bbmpc_handle h, const float* states, const float* action_sequences, int32_t batch,
                                       int32_t horizon, const float* eps, float* state_mean, float* state_std,
                                       float* reward_mean, float* reward_std, float* particle_states, float* particle_rewards);
int bbmpc_predict_trajectory_particles_dev(bbmpc_handle h, const float* d_states, const float* d_action_sequences, int32_t batch,
                                           int32_t horizon, const float* d_eps, float* d_state_mean, float* d_state_std,
                                           float* d_reward_mean, float* d_reward_std, float* d_particle_states,
                                           float* d_particle_rewards);
/* The same with nearest-rank quantiles over the particles: bbmpc_predict_trajectory_particles' arguments, then num_levels in
 * [1, 8], ranks [num_levels] (a HOST array in both variants, each rank in [0, num_particles)) and the outputs
 * state_quantiles [B,L,Hq,S], reward_quantiles [B,L,Hq] (L = num_levels).  With the stable rank of bbmpc_set_particle_risk
 * among the P particle values x[b,:,t,f],
 *     state_quantiles[b,l,t,f] = x[b,p,t,f] of the particle p whose rank is ranks[l]
 * -- an element of the particle tensor, bit for bit: rank 0 is the minimum over the particles, P - 1 the maximum, P = 1
 * returns the particle; the level tau in (0, 1] of the nearest-rank definition is rank ceil(tau P) - 1.  The same for the
 * rewards.  The draws, the trajectories and the moments are those of bbmpc_predict_trajectory_particles (same eps, same
 * bits); all eight outputs are optional, not all may be NULL.  Per-step values are not NaN-filtered here: where a NaN is
 * among the P values their ranks mean nothing and so do the quantiles of that element (nothing special is propagated).
 * Refusals, before anything is allocated, copied or launched: everything bbmpc_predict_trajectory_particles refuses;
 * BBMPC_E_INVALID: num_levels outside [1, 8], ranks NULL, a rank outside [0, num_particles); BBMPC_E_UNSUPPORTED:
 * B * L * Hq * S >= 2^31. */
int bbmpc_predict_trajectory_quantiles(bbmpc_handle h, const float* states, const float* action_sequences, int32_t batch,
                                       int32_t horizon, const float* eps, float* state_mean, float* state_std,
                                       float* reward_mean, float* reward_std, float* particle_states, float* particle_rewards,
                                       int32_t num_levels, const int32_t* ranks, float* state_quantiles, float* reward_quantiles);
int bbmpc_predict_trajectory_quantiles_dev(bbmpc_handle h, const float* d_states, const float* d_action_sequences, int32_t batch,
                                           int32_t horizon, const float* d_eps, float* d_state_mean, float* d_state_std,
                                           float* d_reward_mean, float* d_reward_std, float* d_particle_states,
                                           float* d_particle_rewards, int32_t num_levels, const int32_t* ranks,
                                           float* d_state_quantiles, float* d_reward_quantiles);

/* Temporally correlated ("colored") sampling for CEM and PI2.  mix is a row-major [H, H] matrix M
 * (H = planning_horizon) shared by all agents and action dimensions; with z[n,a,s,u] the unit truncated-normal draws of
 * an iteration (stream BBMPC_NOISE_TRUNC_NORMAL, keyed as always; an injected tensor of that kind is the z that is mixed,
 * bbmpc_dump_noise still returns the unmixed z) the candidates become
 *     y[n,a,t,u] = sum over s = 0 .. H-1, ascending, in fp32, of M[t,s] * z[n,a,s,u]
 *     x[n,a,t,u] = y * sigma[a,t,u] + mean[a,t,u]
 * with the sigma and mean the iteration would use anyway; M = identity gives the bits of the uncorrelated draw.  CEM: x is
 * clipped to [action_low, action_high] (a mixed draw is not bounded by two sigma); the clipped x is rolled out, stored and
 * seen by the refit, no penalty.  PI2: unchanged from there on (clip, squared-norm penalty, feasible samples stored).
 * iCEM's power-law noise, smooth-MPPI and Ornstein-Uhlenbeck exploration are all a lower-triangular M (the Cholesky factor
 * of the wanted autocovariance; blackbox_mpc_amd/utils/colored_noise.py builds two).
 * mix != NULL, count == H * H installs M: copied to the device on the handle's stream, the call waits for the copy.
 * mix == NULL, count == 0 removes it and restores every path bit for bit.  While a matrix is installed, control steps are
 * routed as bbmpc_set_trace routes them (one launch sequence per iteration: no resident, fused or graph-replayed form): same
 * rule on every model, slower paths.  Like the other setters the call stops a resident control-step kernel first and
 * invalidates the captured step graph.  Survives bbmpc_reset.
 * Refusals, before anything is allocated, copied or launched (the handle stays as it was): BBMPC_E_UNSUPPORTED: an
 * optimizer other than CEM or PI2, a sharded population, H * dim_u > 636 (the kernel's LDS tile); BBMPC_E_INVALID: count
 * != H * H (or != 0 with mix == NULL), a non-finite element.  No counterpart in the reference. */
int bbmpc_set_sampling_correlation(bbmpc_handle h, const float* mix, int64_t count);
/* *installed = 1 while a matrix is installed, else 0. */
int bbmpc_get_sampling_correlation(bbmpc_handle h, int32_t* installed);

/* Elite carry-over for CEM, the second half of iCEM.  With k = num_elite, N = population_size,
 * E_i[a] the sorted elite list of iteration i of agent a (best first, ties by lower index) and X_i[n,a,t,u] the candidates
 * of iteration i as rolled out:
 *   keep:  for i >= 1 within a control step, after the draw of iteration i,
 *              X_i[N - keep + e, a] = X_{i-1}[E_{i-1}[a][e], a]                      e = 0 .. keep-1, bit for bit
 *   shift: with L the last iteration of control step c, after the draw of iteration 0 of control step c + 1,
 *              X_0[N - shift + e, a, t, :] = X_L[E_L[a][e], a, min(t + 1, H - 1), :]   e = 0 .. shift-1, bit for bit
 *          (the elite moved one planning step forward, its last action repeated).
 * The replaced columns are always the last ones; their draws are still made, keyed as always, and then overwritten
 * (bbmpc_dump_noise returns what it returned before).  Everything behind the candidates is untouched: rollout, top-k over
 * all N columns (a carried column can be selected again), refit, smoothing, the action; mean and variance across control
 * steps stay governed by the quirk bits.  The stored elites live in a buffer of the handle's own: bbmpc_evaluate, the
 * predict calls and bbmpc_set_trace between two control steps do not disturb them; bbmpc_reset and an accepted call of
 * this setter drop them (the next control step injects nothing into its first iteration); the setting itself survives
 * bbmpc_reset.  keep = shift = 0 switches it off and restores every path bit for bit.  While it is on, control steps are
 * routed as bbmpc_set_trace routes them (one launch sequence per iteration: no resident, fused or graph-replayed form).
 * Like the other setters the call stops a resident control-step kernel first and invalidates the captured step graph.
 * Refusals, before anything is allocated or launched (the handle, an earlier setting and its stored elites included,
 * stays as it was): BBMPC_E_UNSUPPORTED: an optimizer other than CEM, a sharded population; BBMPC_E_INVALID: keep or shift
 * negative, above num_elite, or not below population_size.  No counterpart in the reference. */
int bbmpc_set_elite_carry(bbmpc_handle h, int keep, int shift);
/* The setting, and *stored = the number of elites currently held for the next control step. */
int bbmpc_get_elite_carry(bbmpc_handle h, int* keep, int* shift, int* stored);

/* Learned policy prior for CEM on a learned model (BBMPC_DYN_MLP): `count` = K closed-loop rollouts of a policy network
 * pi through the learned model replace K sampled candidates of every iteration.  pi is a Dense stack dims[0] = dim_s ->
 * dims[n_layers] = dim_u in bbmpc_set_mlp's layouts (any BBMPC_ACT_* per layer), stats = mean_in [dim_s], std_in [dim_s],
 * mean_out [dim_u], std_out [dim_u] when is_normalized:
 *   pi(s) = y * std_out + mean_out,  y = stack((s - mean_in) / (std_in + 1e-7f))          (y itself when not normalised)
 * For iteration i of control step c, agent a, policy rollout e = 0 .. K-1:
 *   s_0 = state[a];   a_t = clip(pi(s_t) + noise_std * xi[i, a, e, t, :], lo, hi);
 *   s_{t+1} = what bbmpc_predict_next_state computes for (s_t, a_t);   X_i[N - c_i - K + e, a, t, :] = a_t
 * with c_i the carried elites injected in that iteration (bbmpc_set_elite_carry; 0 without): the policy columns sit
 * directly in front of the carried ones.  The draws of the replaced columns are still made, with unchanged keying, and then
 * overwritten; everything behind the candidates (rollout, top-k, refit, smoothing, the action) is untouched.  xi is stream
 * BBMPC_NOISE_POLICY, [iters][A,K,H,U] N(0,1): Philox counter (e, ga * Qk + (j >> 2), control_step, (12 << 16) | iter), ga
 * the global agent id, j = t * dim_u + u, Qk = ceil(H * dim_u / 4), Box-Muller on word pairs -- or injected
 * (bbmpc_inject_noise).  While a network is installed control steps take one launch sequence per iteration, as with
 * bbmpc_set_elite_carry.  n_layers = 0 removes the network and restores routing and outputs bit for bit.  An accepted call
 * settles the handle (a resident control-step kernel is stopped, a captured step graph dropped); a refused one leaves it as
 * it was.  BBMPC_E_UNSUPPORTED: more than 8 layers, a hidden width > 512, an optimizer other than CEM, dynamics other than
 * BBMPC_DYN_MLP, callback plug-ins, an inverse target transform, a sharded population, a model ensemble or log-variance
 * heads (each of the last four also refused by its own setter while a prior is installed), buffers that do not fit the LDS.
 * BBMPC_E_INVALID: NULL pointers, dims[0] != dim_s, dims[n_layers] != dim_u, a width < 1, an unknown activation,
 * is_normalized without stats, noise_std negative or not finite, count < 1, count + max(keep, shift) >= population_size
 * (bbmpc_set_elite_carry checks the same while a prior is installed).  bbmpc_reset keeps the setting. */
int bbmpc_set_policy_prior_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* activations,
                               const float* const* weights, const float* const* biases, int32_t is_normalized,
                               const float* const* stats, int32_t count, float noise_std);
/* The setting; BBMPC_E_STATE (and *count = 0) without a network. */
int bbmpc_get_policy_prior(bbmpc_handle h, int32_t* count, float* noise_std);
/* pi on `batch` rows of states [batch][dim_s] -> actions [batch][dim_u]: no noise, no clip.  BBMPC_E_STATE without a
 * network.  The _dev form takes device pointers and is ordered on the handle's stream. */
int bbmpc_evaluate_policy_prior(bbmpc_handle h, const float* states, int32_t batch, float* actions);
int bbmpc_evaluate_policy_prior_dev(bbmpc_handle h, const float* d_states, int32_t batch, float* d_actions);
/* The K policy rollouts of every agent from states [A][dim_s], by exactly the kernel a control step runs:
 * actions_out [K,A,H,dim_u] (the candidate columns) and states_out [K,A,H,dim_s] (s_1 .. s_H); either may be NULL, not
 * both.  noise: [A,K,H,dim_u] standard normals, or NULL for the handle's BBMPC_NOISE_POLICY stream at the current control
 * step, iteration 0 (equal calls give equal bits).  BBMPC_E_STATE without a network or without bbmpc_set_mlp. */
int bbmpc_predict_policy_rollouts(bbmpc_handle h, const float* states, const float* noise, float* actions_out, float* states_out);
int bbmpc_predict_policy_rollouts_dev(bbmpc_handle h, const float* d_states, const float* d_noise, float* d_actions_out,
                                      float* d_states_out);

/* Closed-loop episode on the device -- counterpart of utils/rollouts.py:60-139 (_sample) with the engine's own
 * model as the environment: T control steps, each feeding its predicted next state back as the next observation;
 * nothing leaves HBM until the end.  records_out is [T][A][U+S+1] (action | next_state | reward) on the host.
 * Equivalent to T calls of bbmpc_optimize with state_{t+1} = next_state_t (no exploration noise). */
int bbmpc_rollout_episode(bbmpc_handle h, const float* start_state, int32_t num_steps, int32_t add_exploration_noise,
                          float* records_out);

/* ---- parity / test hooks ------------------------------------------------ */
/* Replace the engine's Philox draws of `kind` by caller-supplied standard noise
 * (reference layout, see BBMPC_NOISE_*).  count = number of floats.  data == NULL
 * clears the injection for that kind.  Injected tensors are consumed by every
 * subsequent control step until cleared. */
int bbmpc_inject_noise(bbmpc_handle h, int32_t kind, const float* data, int64_t count);
/* Write the standard noise the engine's own Philox scheme produces for (kind, control_step, iteration),
 * in the reference layout -- lets tests check the generator against its documented definition. */
int bbmpc_dump_noise(bbmpc_handle h, int32_t kind, int32_t control_step, int32_t iteration, float* out,
                     int64_t count);
/* Enable per-iteration trace capture (costs extra device copies; off by default). */
int bbmpc_set_trace(bbmpc_handle h, int32_t enabled);
int bbmpc_get_trace(bbmpc_handle h, int32_t iteration, int32_t item, void* out, int64_t bytes);
/* Read / write optimizer state tensors by name ("mean","var","pos","vel","pbest","pbest_r",
 * "gbest","gbest_r","m","sigma","C","B","D","p_sigma","p_C"), reference layout.  Settable: "prev_mean", "var0",
 * and with CMA-ES "C" (G*n*n). */
int bbmpc_get_state(bbmpc_handle h, const char* name, float* out, int64_t count);
int bbmpc_set_state(bbmpc_handle h, const char* name, const float* data, int64_t count);

/* ---- measurement -------------------------------------------------------- */
/* When enabled the handle brackets launches of its dominant (rollout) kernel with HIP events on the launch
 * stream: enabled = 1 every launch, enabled = n > 1 every n-th launch (an event pair costs a few microseconds
 * of stream time, which matters when the whole control step is ~50 us); bbmpc_get_profile returns the
 * accumulated device time and the number of bracketed launches since the last call and resets them. */
int bbmpc_set_profiling(bbmpc_handle h, int32_t enabled);
int bbmpc_get_profile(bbmpc_handle h, double* rollout_ms_total, int64_t* rollout_launches,
                      const char** kernel_name);
/* The dominant kernel of the last control step with its template arguments, spelt as rocprofv3 prints kernel names minus the
 * leading "void " (e.g. "k_fused_pendulum<2, true, true, 2, 1, false>": optimizer, samples in LDS, carried-angle model,
 * noise source, trajectories per lane, resident) when the engine holds several instantiations of it, the plain name
 * otherwise.  bench.py attaches the committed PMC counters (profiles/) to a measurement by THIS name, so that a counter of
 * the BBMPC_STRICT_MATH or the resident instantiation can never be divided by the default instantiation's time.
 * The string lives in the handle and changes with the next control step. */
int bbmpc_profile_instantiation(bbmpc_handle h, const char** kernel_instantiation);
/* Block until everything enqueued on the handle's stream (and its communication stream) has finished. */
int bbmpc_synchronize(bbmpc_handle h);

/* ---- multi-GPU: the agent-sharded path's one exchange ------------------------
 * One process per GPU, each handle owning agents [agent_offset, agent_offset + num_agents) of num_agents_global
 * (bbmpc_config).  Nothing on the optimisation path crosses GPUs; per control step the packed records
 * [num_agents, dim_u + dim_s + 1] are all-gathered (RCCL over xGMI) so every rank holds every agent's action /
 * predicted next state / predicted reward.  The reference has no counterpart: its agents are a batch dimension of a
 * single process (optimizers/optimizer_base.py:59-94 returns all agents' results at once); the gathered array is
 * exactly that return value, reassembled.
 *
 *   rank 0: bbmpc_comm_unique_id(id)  -> ship the BBMPC_COMM_ID_BYTES to every rank (any side channel)
 *   all   : bbmpc_comm_init(h, id, nranks, rank)              (collective; librccl is bound at run time)
 *   step t: bbmpc_gather_wait(h, t & 1, 0);                    the gather that last used this slot's buffers is done
 *           bbmpc_optimize_dev(h, ..., d_records[t & 1], ...);
 *           bbmpc_gather_records_dev(h, d_records[t & 1], d_gathered[t & 1], num_agents * record_width, t & 1);
 * The collective runs on the handle's own stream and overlaps the next control step; rows of d_gathered are in
 * global agent order when every rank has the same num_agents.  bbmpc_gather_wait with host_block != 0 blocks the
 * calling thread until the slot's gathered array can be read. */
#define BBMPC_COMM_ID_BYTES 128
int bbmpc_comm_unique_id(void* out, int64_t bytes);
int bbmpc_comm_init(bbmpc_handle h, const void* unique_id, int32_t nranks, int32_t rank);
/* The same communicator for `nranks` handles of ONE process on ONE device, without RCCL (which refuses two ranks on a GPU):
 * handles that pass the same `group_key` form the group, rank = 0 .. nranks-1 (at most 16).  Its all-gather is copies and events on the callers'
 * streams around a HOST rendezvous of the ranks (csrc/comm.hpp): every rank must be driven by its own host thread, as ranks
 * are processes elsewhere, and a rank that does not show up within 60 s fails the others' call.  Everything else -- record gathers, the
 * per-iteration exchanges of a sharded population, bbmpc_comm_info / _destroy -- works as with bbmpc_comm_init.  It exists so
 * that the rank > 0 / nranks > 1 paths run on a one-GPU box (tests/test_gpu_local_ranks.py), and for several handles sharing a
 * device.  At most 1 MiB
 * per rank and operation.  No counterpart in the reference. */
int bbmpc_comm_init_local(bbmpc_handle h, uint64_t group_key, int32_t nranks, int32_t rank);
int bbmpc_gather_records_dev(bbmpc_handle h, const float* d_records, float* d_gathered, int64_t count_per_rank,
                             int32_t slot);
/* bbmpc_optimize_dev + bbmpc_gather_records_dev in one call (count = num_agents * record width): lets a control
 * step that is a single kernel launch carry the "records ready" event on its own dispatch packet instead of a
 * separate event record on the launch stream. */
int bbmpc_optimize_gather_dev(bbmpc_handle h, const float* d_state, int32_t time_step, int32_t add_exploration_noise,
                              float* d_records, float* d_next_state, float* d_gathered, int32_t slot);
/* MPCPolicy.act (policies/mpc_policy.py:124-172) of ONE RANK of an agent-sharded run: bbmpc_optimize for the local
 * agents (host buffers, synchronous) + the all-gather of their records into d_gathered [num_agents_global, U+S+1]
 * (device memory), enqueued on the communication stream and overlapped with the caller's next control step. */
int bbmpc_optimize_gather(bbmpc_handle h, const float* state, int32_t time_step, int32_t add_exploration_noise,
                          float* action, float* next_state, float* reward, float* d_gathered, int32_t slot);
/* ncclCommCount / ncclCommUserRank of the handle's communicator and the hand-off mode in use
 * (1 = sequence numbers in signal memory, 0 = events); any out pointer may be NULL. */
int bbmpc_comm_info(bbmpc_handle h, int32_t* nranks, int32_t* rank, int32_t* sync_mode);
int bbmpc_gather_wait(bbmpc_handle h, int32_t slot, int32_t host_block);
int bbmpc_comm_destroy(bbmpc_handle h);

/* ---- training a Dense stack ------------------------------------------------------------------------
 * Counterpart of SystemDynamicsHandler._training_algorithm (dynamics_handlers/system_dynamics_handler.py:243-290) with
 * DeterministicMLP.get_loss (Keras MeanSquaredError) and tf.keras.optimizers.{Adam, SGD, RMSprop}(learning_rate) at their
 * TF-2.0 defaults, in hand-written kernels (csrc/kernels_train.hpp).  A trainer is its own opaque handle, independent of
 * bbmpc_handle: training needs no planning configuration.  One trainer = one caller thread at a time.
 *
 * The rule.  Rows are already normalised: train_in [n_train][dims[0]], train_out [n_train][dims[n_layers]], val_in, val_out.
 * One epoch takes the batches perm[s .. s + B), s = 0, B, 2B, ... and drops the remainder.  Loss = mean over the batch's
 * B * dims[n_layers] elements of (f(x) - y)^2.  Per batch one update:
 *   BBMPC_TRAIN_ADAM     m = 0.9 m + 0.1 g;  v = 0.999 v + 0.001 g^2;  lr_t = lr sqrt(1 - 0.999^t) / (1 - 0.9^t) (the powers
 *                        carried in double);  w -= lr_t m / (sqrt(v) + 1e-7)
 *   BBMPC_TRAIN_SGD      w -= lr g
 *   BBMPC_TRAIN_RMSPROP  v = 0.9 v + 0.1 g^2;  w -= lr g / (sqrt(v) + 1e-7)
 * m, v and t belong to the trainer and go on from one bbmpc_trainer_fit to the next.  train_loss_out[e] = mean of epoch e's
 * batch losses (NaN without a full batch); val_loss_out[e] = mean of the per-batch MSEs over the floor(n_val / B) full batches
 * val[0 .. B), val[B .. 2B), ... after the epoch (NaN without one).  Equal calls from equal starts give equal bits.
 * Log-variance heads / Gaussian NLL: bbmpc_trainer_create_gaussian, below.
 *
 * Layouts as bbmpc_set_mlp: Dense kernels [in, out] row-major, biases [out], dims has n_layers + 1 entries (so the widths
 * chain by construction), any BBMPC_ACT_* code per layer.  device: HIP ordinal, -1 = current.
 * Refused before anything is allocated -- BBMPC_E_UNSUPPORTED: n_layers > 8, a width > 512, a network whose LDS carve
 * (bbmpc_trainer_lds_bytes) passes 159 KiB; BBMPC_E_INVALID: NULL pointers, n_layers < 1, a width < 1, an unknown activation or
 * rule, learning_rate not finite or not positive; BBMPC_E_NO_DEVICE. */
#define BBMPC_TRAIN_ADAM    1
#define BBMPC_TRAIN_SGD     2
#define BBMPC_TRAIN_RMSPROP 3
typedef struct bbmpc_trainer_s* bbmpc_trainer;
int bbmpc_trainer_create(bbmpc_trainer* out, int32_t device, int32_t n_layers, const int32_t* dims, const int32_t* activations,
                         const float* const* weights, const float* const* biases, int32_t rule, float learning_rate);
int bbmpc_trainer_destroy(bbmpc_trainer t);     /* NULL is fine */
/* The step kernel's LDS carve in bytes, 4 * (256 * (sum_{l=0..L} T_l + sum over swish layers of T_{l+1} + max_l T_l) + 1088),
 * T_l = ceil(dims[l] / 16).  Host arithmetic only: no device needed. */
int bbmpc_trainer_lds_bytes(int32_t n_layers, const int32_t* dims, const int32_t* activations, int64_t* bytes);
/* The dataset: host rows, copied to device memory once.  Replaces the previous one.  n_val may be 0. */
int bbmpc_trainer_set_data(bbmpc_trainer t, const float* train_in, const float* train_out, int32_t n_train, const float* val_in,
                           const float* val_out, int32_t n_val);
/* `epochs` epochs at batch size B.  perms: [epochs][n_train] int32 row indices, one permutation per epoch, or NULL -- then the
 * library draws them from `seed`: Fisher-Yates from the top, j = floor(u (i + 1) / 2^64) for i = n_train - 1 .. 1 with u the
 * next splitmix64 output, the generator's state starting at seed ^ (0xD1B54A32D192ED03 * (epoch + 1)).  Every epoch's
 * permutation is on the device before the first step; an epoch is nothing but kernel launches on the trainer's stream, and
 * the losses [epochs] are read once at the end.  BBMPC_E_STATE before bbmpc_trainer_set_data; BBMPC_E_UNSUPPORTED: batch_size
 * outside [1, 4096]; BBMPC_E_INVALID: epochs < 1, NULL outputs, a permutation entry outside [0, n_train).  A refused call
 * leaves the trainer as it was. */
int bbmpc_trainer_fit(bbmpc_trainer t, int32_t epochs, int32_t batch_size, const int32_t* perms, uint64_t seed, float* train_loss_out,
                      float* val_loss_out);
/* The current parameters (before any fit: the initial ones, bit for bit). */
int bbmpc_trainer_get_params(bbmpc_trainer t, float* const* weights, float* const* biases);
/* Per-output RMS of (out - prediction) over n >= 1 host rows: rms_out [dims[n_layers]]. */
int bbmpc_trainer_residual_rms(bbmpc_trainer t, const float* in, const float* out, int32_t n, float* rms_out);
/* Test window: loss and gradient of the batch made of training rows idx[0 .. batch_size), by exactly the step's kernels,
 * without updating anything.  grads_out holds every parameter in the order W_0 .. W_{L-1} ([in][out] row-major), b_0 ..
 * b_{L-1}.  Refusals as bbmpc_trainer_fit; an index outside [0, n_train) is BBMPC_E_INVALID. */
int bbmpc_trainer_gradients(bbmpc_trainer t, const int32_t* idx, int32_t batch_size, float* grads_out, float* loss_out);

/* ---- training the members of an ensemble in one launch sequence -----------------------------------
 * A trainer may hold n_members equally shaped networks, 1 <= n_members <= BBMPC_MAX_ENSEMBLE_MEMBERS (8).  They are fitted
 * side by side: the member index is a second grid dimension of every training kernel, so a step of all members is the two
 * launches a step of one member is.  Member e has its own parameters, optimizer state and losses and shares nothing but the
 * dataset, which is on the device once; its arithmetic and summation order are the single trainer's, whatever n_members is
 * and whatever the other members hold (NaN included): member e's results are, bit for bit, those of a bbmpc_trainer_create
 * trainer given member e's start weights, rows and permutations.
 *
 * weights / biases: [n_members * n_layers] pointers, member major (member e's layer l at [e * n_layers + l]); the other
 * arguments and refusals as bbmpc_trainer_create, and BBMPC_E_UNSUPPORTED for n_members outside [1, 8].  n_members = 1 is
 * legal and is a bbmpc_trainer_create trainer.  bbmpc_trainer_set_data and bbmpc_trainer_destroy serve both kinds; on a
 * trainer with n_members > 1 bbmpc_trainer_fit, _get_params, _residual_rms and _gradients are BBMPC_E_STATE, with a message
 * that names the call to use. */
int bbmpc_trainer_create_ensemble(bbmpc_trainer* out, int32_t device, int32_t n_members, int32_t n_layers, const int32_t* dims,
                                  const int32_t* activations, const float* const* weights, const float* const* biases, int32_t rule,
                                  float learning_rate);
/* The members' training rows (a bootstrap resample is an index map, not a copy): rows [n_members][n_train] int32 into the
 * training rows bbmpc_trainer_set_data uploaded -- member e trains as if its dataset were train[rows[e][0]], train[rows[e][1]],
 * ...  NULL, or never called: the identity for every member.  A new bbmpc_trainer_set_data resets it.  BBMPC_E_STATE before
 * bbmpc_trainer_set_data; BBMPC_E_INVALID: an entry outside [0, n_train) (the map then stays as it was). */
int bbmpc_trainer_set_member_rows(bbmpc_trainer t, const int32_t* rows);
/* bbmpc_trainer_fit for every member at once.  perms: [n_members][epochs][n_train] int32, member e's permutation of epoch k
 * indexing ITS rows: position pos of the epoch is training row rows[e][perms[e][k][pos]] (the two maps are composed on the
 * host into one index array [n_members][epochs][n_train]).  NULL: member e draws what bbmpc_trainer_fit draws from the seed
 * seed ^ (0x9E3779B97F4A7C15 * e mod 2^64) -- member 0 from `seed` itself.  train_loss_out / val_loss_out:
 * [n_members][epochs]; the validation rows are shared.  Per step two launches and per epoch the validation pair, each for
 * all members; no host synchronisation inside the fit.  Refusals as bbmpc_trainer_fit, and BBMPC_E_UNSUPPORTED where
 * n_members * epochs * n_train >= 2^31. */
int bbmpc_trainer_fit_ensemble(bbmpc_trainer t, int32_t epochs, int32_t batch_size, const int32_t* perms, uint64_t seed,
                               float* train_loss_out, float* val_loss_out);
/* bbmpc_trainer_get_params of one member; BBMPC_E_INVALID: member outside [0, n_members). */
int bbmpc_trainer_get_member_params(bbmpc_trainer t, int32_t member, float* const* weights, float* const* biases);
/* bbmpc_trainer_residual_rms of every member on the same n >= 1 host rows (uploaded once): rms_out [n_members][dims[n_layers]]. */
int bbmpc_trainer_residual_rms_ensemble(bbmpc_trainer t, const float* in, const float* out, int32_t n, float* rms_out);

/* ---- weight decay, early stopping, best-weights restore ---------------------------------------------
 * Three settings of a trainer of either kind.  They hold from one fit to the next until they are set again; a trainer that
 * never sets them, or sets them to (NULL, patience 0, restore_best 0), fits bit for bit as described above, with the same
 * launches.  Reported losses stay the data term (MSE) and bbmpc_trainer_gradients the data gradient.
 *
 * Weight decay: one lambda_l >= 0 per layer, on the kernels W_l only, never on biases.  w0 is W_l before the step, g the
 * data gradient; every line is one float32 operation:
 *   BBMPC_TRAIN_DECAY_L2         g' = fma(lambda_l, w0, g); the rule then runs on g' exactly as it runs on g
 *   BBMPC_TRAIN_DECAY_DECOUPLED  w1 = the rule's result on g; w = fma(-(lr lambda_l), w0, w1), lr the BASE rate (not Adam's
 *                                lr_t), the product lr lambda_l rounded to float32 once (AdamW-style)
 * A lambda_l of 0 adds no operation: that layer's bits are the undecayed ones.
 *
 * Monitoring is on with patience > 0 or restore_best != 0, and needs a validation loss: a fit whose n_val holds no full
 * batch is then BBMPC_E_STATE, before anything runs.  Per member, after every epoch k, on the device:
 *   v_k improves if v_k < best - min_delta (float32; best starts at +inf; a NaN v_k never improves)
 *   improvement:  best = v_k, best_epoch = k, wait = 0, the member's parameters are copied to a snapshot
 *   otherwise:    wait += 1
 *   patience > 0 and wait >= patience: the member stops after epoch k
 * A stopped member runs no further step (its launches are still enqueued: the workgroups return at once, and there is no host
 * synchronisation inside the fit); its train_loss_out / val_loss_out entries of the epochs it did not run are NaN.  At the
 * end of the fit, with restore_best and best_epoch >= 0, the member's parameters become the snapshot; m, v, the running
 * powers and the step count stay as they are (Keras restore_best_weights restores weights only); with best_epoch = -1 the
 * current parameters stay.  Members monitor, stop and restore independently of each other.
 *
 * bbmpc_trainer_set_weight_decay: decay [n_layers], NULL = off.  BBMPC_E_INVALID, the settings then as they were: an
 * unknown mode, a negative or non-finite decay.
 * bbmpc_trainer_set_early_stopping: BBMPC_E_INVALID for patience < 0 or a negative or non-finite min_delta.
 * bbmpc_trainer_get_fit_report: the last fit, each array [n_members]: epochs_run (epochs, or fewer for a stopped member),
 * best_epoch (-1: none, or no monitoring) and best_val (NaN then).  Host values kept from the fit's one read at its end.
 * BBMPC_E_STATE before any fit; BBMPC_E_INVALID for a NULL array. */
#define BBMPC_TRAIN_DECAY_L2        0
#define BBMPC_TRAIN_DECAY_DECOUPLED 1
int bbmpc_trainer_set_weight_decay(bbmpc_trainer t, const float* decay, int32_t mode);
int bbmpc_trainer_set_early_stopping(bbmpc_trainer t, int32_t patience, float min_delta, int32_t restore_best);
int bbmpc_trainer_get_fit_report(bbmpc_trainer t, int32_t* epochs_run, int32_t* best_epoch, float* best_val);

/* ---- log-variance heads: the Gaussian negative log-likelihood ---------------------------------------
 * A trainer whose members carry a second last Dense layer on the last hidden activation h = y_{L-1} (the input when n_layers
 * = 1), the log-variance head of ProbabilisticMLP / EnsembleMLP(probabilistic=True) (bbmpc_set_mlp_logvar_head), fitted
 * together with the mean network on
 *   mu = act_{L-1}(h W_{L-1} + b_{L-1});   z = h W_v + b_v
 *   lv1 = max_lv - softplus(max_lv - z);   lv = min_lv + softplus(lv1 - min_lv)
 *   loss = mean over the batch's B * O elements of (mu - y)^2 exp(-lv) + lv,   O = dims[n_layers]
 *   d loss / d mu = 2 (mu - y) exp(-lv) / (B O)
 *   d loss / d z  = (1 - (mu - y)^2 exp(-lv)) sigmoid(lv1 - min_lv) sigmoid(max_lv - z) / (B O)
 * W_v [dims[n_layers - 1]][O] and b_v [O] are parameters like any other (same update rules, m, v, powers); in the parameter
 * vector they follow b_{L-1}.  Weight decay treats W_v as a kernel with the last layer's lambda and b_v as a bias.  The bounds
 * are fixed.  softplus, exp and the logistic function are evaluated in their accurate float32 forms.
 *
 * weights / biases: [n_members * n_layers] pointers, member major; head_weights / head_biases: [n_members] pointers;
 * min_logvar / max_logvar: [O], shared by the members.  n_members = 1 is the single model.  Refusals as
 * bbmpc_trainer_create_ensemble, the LDS limit on bbmpc_trainer_lds_bytes_gaussian; BBMPC_E_INVALID also for a NULL head
 * array and for bounds that are not finite, not inside [-40, 40] or have min_logvar > max_logvar.
 *
 * On such a trainer every other bbmpc_trainer_* call works as described above (the single-member ones with n_members = 1), and
 * every loss is the NLL: train_loss_out, val_loss_out (mean of the per-batch NLLs), what the monitor compares, best_val, and
 * bbmpc_trainer_gradients' loss, whose grads_out holds n_params = the mean network's + dims[n_layers - 1] * O + O floats, W_v
 * and b_v last.  bbmpc_trainer_residual_rms(_ensemble) stays the mean network's residual.  Member e of n_members is, bit for
 * bit, the single Gaussian trainer with its start parameters, rows and permutations. */
int bbmpc_trainer_create_gaussian(bbmpc_trainer* out, int32_t device, int32_t n_members, int32_t n_layers, const int32_t* dims,
                                  const int32_t* activations, const float* const* weights, const float* const* biases,
                                  const float* const* head_weights, const float* const* head_biases, const float* min_logvar,
                                  const float* max_logvar, int32_t rule, float learning_rate);
/* Member `member`'s current head: head_weights_out [dims[n_layers - 1]][O], head_bias_out [O].  BBMPC_E_STATE on a trainer
 * without a head; BBMPC_E_INVALID: NULL outputs, member outside [0, n_members). */
int bbmpc_trainer_get_logvar_head(bbmpc_trainer t, int32_t member, float* head_weights_out, float* head_bias_out);
/* bbmpc_trainer_lds_bytes with the head's tile array: 4 * (256 * (sum_{l=0..L} T_l + sum over swish layers of T_{l+1} +
 * max_l T_l + T_L) + 1088).  Host arithmetic only: no device needed. */
int bbmpc_trainer_lds_bytes_gaussian(int32_t n_layers, const int32_t* dims, const int32_t* activations, int64_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* BBMPC_H */
