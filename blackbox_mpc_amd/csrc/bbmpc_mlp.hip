// Learned-dynamics half of the engine (DeterministicMLP, dynamics_functions/deterministic_mlp.py:5-51 behind
// SystemDynamicsHandler.process_input / process_output): weight packing and the choice + launch of the MFMA rollout
// kernels (kernels_mlp*.hpp).  A translation unit of its own: the template kernels are instantiated here only.
#define BBMPC_TU_MLP
#include <cmath>
#include <type_traits>

#include "abi_util.hpp"
#include "engine.hpp"
#include "engine_util.hpp"
#include "kernels_reward_mlp.hpp"
#include "kernels_return_shaping.hpp"
#include "kernels_mlp_traj.hpp"
#include "kernels_mlp_particles.hpp"
#include "kernels_mlp_traj_particles.hpp"
#include "kernels_policy_prior.hpp"
#include "kernels_plan_grad.hpp"
#include "kernels_plan_refine.hpp"

namespace bbmpc {

void bbmpc_tu_mlp_upload_tnq(const float2* table) { tnq_upload(table); }

static_assert(ACT_SIGMOID == BBMPC_ACT_SIGMOID && ACT_ELU == BBMPC_ACT_ELU && ACT_SWISH == BBMPC_ACT_SWISH &&
                  ACT_RELU6 == BBMPC_ACT_RELU6, "activations.hpp and bbmpc.h disagree on the activation codes");

// ------------------------------------------------------------------------------------------------
// operand packing (bbmpc_set_mlp for the handle's model, bbmpc_set_mlp_ensemble per member)
// ------------------------------------------------------------------------------------------------
// Hidden features are internal, so their order inside a tile is free.  When the last tile of a hidden layer
// holds <= 8 features (200 units = 12 tiles + 8) they are put into the slots 4g + {0, 1}: as the next layer's
// K tile that leaves MFMAs 2 and 3 (k = 4g + 2, 4g + 3) with nothing but zeros, and the pipelined kernel
// skips them.  slot -> feature (or -1 = padding); inputs (layer 0) and outputs (last layer) keep their order.
static int mlp_feature_of_slot(const MlpDesc& d, int layer_of_feature, int slot) {
    const int width = d.dims[layer_of_feature], tiles = (width + 15) / 16, t = slot >> 4, q = slot & 15;
    if (layer_of_feature >= 1 && layer_of_feature < d.n_layers && t == tiles - 1 && d.half_tail[layer_of_feature]) {
        if ((q & 3) >= 2) return -1;
        const int f = 16 * t + 2 * (q >> 2) + (q & 3);
        return f < width ? f : -1;
    }
    return slot < width ? slot : -1;
}

// Dense layer l of a network of d's shape (dims, tiles, half_tail): kernel w [in][out] and bias b [out] ->
//   wp [OT][IT][4][64]    MFMA operand order (MlpDesc::wpack)
//   w4 [OT][IT][64][4]    the same operands with a lane's four A operands of a k tile side by side (generic kernel)
//   bp [OT][64][4]        biases in accumulator order (MlpDesc::bpack)
static void mlp_pack_layer(const MlpDesc& d, int l, const float* w, const float* b, std::vector<float>& wp, std::vector<float>& w4,
                           std::vector<float>& bp) {
    const int M = d.dims[l + 1], IT = d.tiles[l], OT = d.tiles[l + 1];
    wp.assign((size_t)OT * IT * 256, 0.0f);
    bp.assign((size_t)OT * 256, 0.0f);
    for (int ot = 0; ot < OT; ++ot) {
        for (int it = 0; it < IT; ++it)
            for (int s = 0; s < 4; ++s)
                for (int ln = 0; ln < 64; ++ln) {
                    const int k = mlp_feature_of_slot(d, l, it * 16 + 4 * (ln >> 4) + s), o = mlp_feature_of_slot(d, l + 1, ot * 16 + (ln & 15));
                    if (k >= 0 && o >= 0) wp[(((size_t)ot * IT + it) * 4 + s) * 64 + ln] = w[(size_t)k * M + o];
                }
        for (int ln = 0; ln < 64; ++ln)
            for (int r = 0; r < 4; ++r) {
                const int o = mlp_feature_of_slot(d, l + 1, ot * 16 + (ln >> 4) * 4 + r);
                if (o >= 0) bp[((size_t)ot * 64 + ln) * 4 + r] = b[o];
            }
    }
    w4.resize(wp.size());
    for (size_t t = 0; t < (size_t)OT * IT; ++t)
        for (int s = 0; s < 4; ++s)
            for (int ln = 0; ln < 64; ++ln) w4[(t * 64 + ln) * 4 + s] = wp[(t * 4 + s) * 64 + ln];
}

// ------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------
void Engine::set_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                     int is_normalized, const float* const* stats) {
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_STATE, "handle was not created with BBMPC_DYN_MLP");
    REQUIRE(n_layers >= 1 && n_layers <= MLP_MAX_LAYERS, BBMPC_E_UNSUPPORTED, "1..8 Dense layers are supported");
    REQUIRE(dims && acts && w && b, BBMPC_E_INVALID, "null argument");
    REQUIRE(dims[0] == S + U && dims[n_layers] == S, BBMPC_E_INVALID, "MLP must map dim_S+dim_U -> dim_S");
    HIP_CHECK(hipStreamSynchronize(stream));
    memset(&mlp, 0, sizeof(mlp));
    ens_E = 0;                                  // (the shape may change: bbmpc_set_mlp_ensemble installs the members again)
    lv_heads = 0;                               // (... and bbmpc_set_mlp_logvar_head the heads)
    mlp.n_layers = n_layers;
    int hidden_tiles = 1;
    for (int l = 0; l <= n_layers; ++l) {
        REQUIRE(dims[l] >= 1, BBMPC_E_INVALID, "layer width must be >= 1");
        mlp.dims[l] = dims[l];
        mlp.tiles[l] = (dims[l] + 15) / 16;
        if (l >= 1 && l < n_layers) hidden_tiles = std::max(hidden_tiles, mlp.tiles[l]);
    }
    REQUIRE(hidden_tiles <= 16 * MLP_TMAX, BBMPC_E_UNSUPPORTED, "hidden width > 512 not supported");
    REQUIRE(mlp.tiles[0] <= 8 && mlp.tiles[n_layers] <= 4, BBMPC_E_UNSUPPORTED, "dim_S+dim_U <= 128 and dim_S <= 64 supported");
    mlp_nw = std::min(16, hidden_tiles);
    for (int l = 1; l < n_layers; ++l) {
        const int tail = dims[l] - 16 * (mlp.tiles[l] - 1);
        mlp.half_tail[l] = (tail <= 8 && !sw.mlp_no_half_tail) ? 1 : 0;
    }
    for (int l = 0; l < n_layers; ++l) {
        REQUIRE(acts[l] >= BBMPC_ACT_NONE && acts[l] <= BBMPC_ACT_RELU6, BBMPC_E_INVALID, "unknown activation");
        REQUIRE(w[l] && b[l], BBMPC_E_INVALID, "null weight/bias pointer");
        mlp.act[l] = acts[l];
        const int K = dims[l], M = dims[l + 1];
        std::vector<float> wp, w4, bp;
        mlp_pack_layer(mlp, l, w[l], b[l], wp, w4, bp);
        upload(d_wpack[l], wp);
        upload(d_wpack4[l], w4);
        upload(d_bpack[l], bp);
        upload(d_wraw[l], std::vector<float>(w[l], w[l] + (size_t)K * M));
        upload(d_braw[l], std::vector<float>(b[l], b[l] + M));
        {   // quad-mode operand order [k/4][Mp][4]; the k/4 axis is zero padded to a multiple of 64 groups so that the
            // kernels can load a fixed number of groups per lane without bounds (group 63 of a <= 252-input layer is a zero row)
            const int Mp = (M + 63) & ~63, KG = ((K + 3) / 4 + 63) & ~63;
            std::vector<float> wq((size_t)KG * Mp * 4, 0.0f);
            for (int kk = 0; kk < K; ++kk)
                for (int o = 0; o < M; ++o) wq[((size_t)(kk >> 2) * Mp + o) * 4 + (kk & 3)] = w[l][(size_t)kk * M + o];
            upload(d_wq4[l], wq);
            if (l == 0 && S <= 20 && U <= 8) {
                // k_rollout_mlp_q4s keeps five state groups and two action groups whatever dim_S is: the state rows padded to 20
                std::vector<float> ws((size_t)KG * Mp * 4, 0.0f);
                for (int kk = 0; kk < K; ++kk) {
                    const int kp = kk < S ? kk : 20 + (kk - S);
                    for (int o = 0; o < M; ++o) ws[((size_t)(kp >> 2) * Mp + o) * 4 + (kp & 3)] = w[l][(size_t)kk * M + o];
                }
                upload(d_wq4s0, ws);
            }
        }
        {   // optional bf16 mode operands: [OT][IT][64] x (4 bf16 hi | 4 bf16 lo), k = 16*it + 4*(lane>>4) + r, row = 16*ot + (lane&15)
            auto bf16_rne = [](float x) -> uint16_t {
                uint32_t u; memcpy(&u, &x, 4);
                u += 0x7fffu + ((u >> 16) & 1u);
                return (uint16_t)(u >> 16);
            };
            auto bf16_f = [](uint16_t h) -> float { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
            const int IT = (K + 15) / 16, OT = (M + 15) / 16;
            std::vector<float> wb((size_t)OT * IT * 64 * 4, 0.0f);          // 16 bytes per lane, kept in a float buffer
            uint16_t* hw = reinterpret_cast<uint16_t*>(wb.data());
            for (int ot = 0; ot < OT; ++ot)
                for (int it = 0; it < IT; ++it)
                    for (int ln = 0; ln < 64; ++ln)
                        for (int r = 0; r < 4; ++r) {
                            // same slot -> feature map as the fp32 operands (the biases come from bpack)
                            const int kk = mlp_feature_of_slot(mlp, l, 16 * it + 4 * (ln >> 4) + r), o = mlp_feature_of_slot(mlp, l + 1, 16 * ot + (ln & 15));
                            const float v = (kk >= 0 && o >= 0) ? w[l][(size_t)kk * M + o] : 0.0f;
                            const uint16_t h = bf16_rne(v), lo = bf16_rne(v - bf16_f(h));
                            uint16_t* d = hw + (((size_t)ot * IT + it) * 64 + ln) * 8;
                            d[r] = h;
                            d[4 + r] = lo;
                        }
            upload(d_wbf[l], wb);
        }
        mlp.wpack[l] = d_wpack[l].p;
        mlp.bpack[l] = d_bpack[l].p;
    }
    {   // k_rollout_mlp_w4 (2..4 Dense layers of at most 32 units, dim_S <= 20, dim_U <= 8): operands in lane order
        bool small = n_layers >= 2 && n_layers <= 4 && S <= 20 && U <= 8;
        for (int l = 1; l < n_layers; ++l) small = small && dims[l] <= 32;
        d_w4pack.release();
        if (small) {
            std::vector<float> wp((size_t)n_layers * W4_OPS * 64, 0.0f);
            for (int l = 0; l < n_layers; ++l)
                for (int op = 0; op < W4_OPS; ++op)
                    for (int ln = 0; ln < 64; ++ln) {
                        const int idx = mlp_w4_operand_index(l, op, ln, dims[l], dims[l + 1], S, U);
                        if (idx >= 0) wp[((size_t)l * W4_OPS + op) * 64 + ln] = op < 16 ? w[l][idx] : b[l][idx];
                    }
            upload(d_w4pack, wp);
        }
    }
    mlp.normalized = is_normalized ? 1 : 0;
    if (is_normalized) {
        REQUIRE(stats, BBMPC_E_INVALID, "normalisation statistics are required when is_normalized != 0");
        upload(d_stats, flatten_stats(stats, S, U));
        float* q = d_stats.p;
        mlp.mean_s = q; q += S;
        mlp.std_s = q; q += S;
        mlp.mean_a = q; q += U;
        mlp.std_a = q; q += U;
        mlp.mean_t = q; q += S;
        mlp.std_t = q;
    }
    mlp_ready = true;
    pg_host[0].keep(n_layers, dims, acts, w, b);        // (plan gradients pack W^T from these at their next call)
    pg_stale[0] = true;
}

// bbmpc_set_mlp_ensemble: E networks of the installed model's shape for the particle rollouts (kernels_mlp_particles.hpp).
// w, b: [E][n_layers] pointers, member-major, in bbmpc_set_mlp's layouts.  Every member is packed on the host before the
// handle is touched, so a refusal leaves it as it was.
void Engine::set_mlp_ensemble(int E, const float* const* w, const float* const* b) {
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_STATE, "handle was not created with BBMPC_DYN_MLP");
    REQUIRE(mlp_ready, BBMPC_E_STATE, "model ensemble: call bbmpc_set_mlp first (the members share its shape and statistics)");
    REQUIRE(E >= 0 && E <= MLP_ENS_MAX, BBMPC_E_UNSUPPORTED, "model ensemble: 0..8 members are supported");
    if (E == 0) {
        invalidate_step_graph();
        ens_E = 0;
        lv_heads = 0;                           // (one head per member: bbmpc_set_mlp_logvar_head comes after this call)
        return;
    }
    REQUIRE(!prior_on(), BBMPC_E_UNSUPPORTED,
            "a model ensemble beside a policy prior (bbmpc_set_policy_prior_mlp): the policy rollout is the noise-free step of one model; "
            "remove the policy network first (n_layers = 0)");
    REQUIRE(!grad_on(), BBMPC_E_UNSUPPORTED,
            "a model ensemble beside gradient refinement (bbmpc_set_grad_refine): the gradient is that of one noise-free model; switch it "
            "off first (steps = 0)");
    REQUIRE(w && b, BBMPC_E_INVALID, "null argument");
    const int L = mlp.n_layers;
    for (int i = 0; i < E * L; ++i) REQUIRE(w[i] && b[i], BBMPC_E_INVALID, "null weight/bias pointer");
    REQUIRE(part_P == 0 || part_P % E == 0, BBMPC_E_INVALID,
            "model ensemble: num_particles = " + std::to_string(part_P) + " is no multiple of num_members = " + std::to_string(E) +
                " (the members must carry equal weight in the mean)");
    std::vector<float> ew[MLP_MAX_LAYERS], eb[MLP_MAX_LAYERS];
    for (int l = 0; l < L; ++l) {
        std::vector<float> wp, w4, bp;
        for (int e = 0; e < E; ++e) {
            mlp_pack_layer(mlp, l, w[e * L + l], b[e * L + l], wp, w4, bp);
            ew[l].insert(ew[l].end(), w4.begin(), w4.end());
            eb[l].insert(eb[l].end(), bp.begin(), bp.end());
        }
    }
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));
    ens_E = 0;
    lv_heads = 0;
    for (int l = 0; l < L; ++l) {
        upload(d_ens_wp4[l], ew[l]);
        upload(d_ens_bp[l], eb[l]);
    }
    ens_E = E;
}

// bbmpc_set_mlp_logvar_head: one log-variance head per model of the particle rollouts (kernels_mlp_particles.hpp) -- the
// handle's model, or each member of its ensemble.  w [num_heads] pointers to [dims[L-1]][S] kernels, b to [S] biases: the last
// layer's layouts.  Packed on the host before the handle is touched, so a refusal leaves it as it was.
void Engine::set_mlp_logvar_head(int num_heads, const float* const* w, const float* const* b, const float* min_logvar,
                                 const float* max_logvar) {
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_STATE, "handle was not created with BBMPC_DYN_MLP");
    REQUIRE(mlp_ready, BBMPC_E_STATE, "log-variance head: call bbmpc_set_mlp first (the head shares the model's last hidden layer)");
    if (num_heads == 0) {
        invalidate_step_graph();
        lv_heads = 0;
        return;
    }
    REQUIRE(!prior_on(), BBMPC_E_UNSUPPORTED,
            "log-variance heads beside a policy prior (bbmpc_set_policy_prior_mlp): the policy rollout is the noise-free step of one model; "
            "remove the policy network first (n_layers = 0)");
    REQUIRE(!grad_on(), BBMPC_E_UNSUPPORTED,
            "log-variance heads beside gradient refinement (bbmpc_set_grad_refine): the gradient is that of one noise-free model; switch "
            "it off first (steps = 0)");
    REQUIRE(w && b && min_logvar && max_logvar, BBMPC_E_INVALID, "null argument");
    const int want = std::max(1, ens_E);
    REQUIRE(num_heads == want, BBMPC_E_INVALID,
            "log-variance head: num_heads = " + std::to_string(num_heads) + " but the handle rolls " + std::to_string(want) +
                " model(s) (one head per ensemble member, one for the model without an ensemble)");
    for (int e = 0; e < num_heads; ++e) REQUIRE(w[e] && b[e], BBMPC_E_INVALID, "null weight/bias pointer");
    for (int s = 0; s < S; ++s)
        REQUIRE(std::isfinite(min_logvar[s]) && std::isfinite(max_logvar[s]) && std::fabs(min_logvar[s]) <= MLP_LOGVAR_ABS_MAX &&
                    std::fabs(max_logvar[s]) <= MLP_LOGVAR_ABS_MAX && min_logvar[s] <= max_logvar[s],
                BBMPC_E_INVALID, "log-variance head: the bounds must be finite, within [-40, 40], with min_logvar <= max_logvar");
    REQUIRE((size_t)mlp_gauss_lds_layout(mlp, U, S, mlp_nw).total * sizeof(float) <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "log-variance head: the partial-sum buffers of the doubled last layer do not fit one CU's LDS next to this network's activations");
    const int L = mlp.n_layers;
    std::vector<float> hw, hb, bounds(min_logvar, min_logvar + S);
    bounds.insert(bounds.end(), max_logvar, max_logvar + S);
    {
        std::vector<float> wp, w4, bp;
        for (int e = 0; e < num_heads; ++e) {
            mlp_pack_layer(mlp, L - 1, w[e], b[e], wp, w4, bp);
            hw.insert(hw.end(), w4.begin(), w4.end());
            hb.insert(hb.end(), bp.begin(), bp.end());
        }
    }
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));
    lv_heads = 0;
    upload(d_lv_wp4, hw);
    upload(d_lv_bp, hb);
    upload(d_lv_bounds, bounds);
    lv_heads = num_heads;
}

// an activation after sigmoid (activations.hpp): the *_ext instantiations, which dispatch over every code; networks of
// none / tanh / relu / sigmoid keep the kernels they always ran
static bool mlp_has_ext_act(const MlpDesc& d) {
    for (int l = 0; l < d.n_layers; ++l)
        if (d.act[l] > BBMPC_ACT_SIGMOID) return true;
    return false;
}

// `hidden` on every hidden layer and a linear output: the networks whose activations some instantiations take at compile time
static bool mlp_is_hidden_act_net(const MlpDesc& d, int hidden) {
    for (int l = 0; l + 1 < d.n_layers; ++l)
        if (d.act[l] != hidden) return false;
    return d.act[d.n_layers - 1] == BBMPC_ACT_NONE;
}
static bool mlp_is_tanh_net(const MlpDesc& d) { return mlp_is_hidden_act_net(d, BBMPC_ACT_TANH); }

// Launch of a kernel that takes one argument struct by value; where it needs more dynamic LDS than the 64 KB default the
// kernel's limit is raised to lds_cap first (ensure_max_lds: once per device and kernel)
template <class Args>
static void launch_args(void (*fn)(Args), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const Args& q, int lds_cap = 159 * 1024) {
    if (lds > 64 * 1024) ensure_max_lds((const void*)fn, lds_cap);
    hipLaunchKernelGGL(fn, grid, block, lds, stream, q);
    HIP_CHECK(hipGetLastError());
}

// What Engine::choose_rollout_mlp decides and Engine::launch_rollout_mlp carries out
struct MlpLaunch {
    using Fn = void (*)(MlpRolloutArgs);
    Fn fn;
    dim3 grid, block;
    size_t lds;                     // dynamic LDS of the launch
    int lds_cap;                    // what the kernel's limit is raised to when lds passes the 64 KB default
    bool raise_lds_always;          // ... or whatever lds is
    const char* name;               // dominant_kernel; nullptr: the caller's stays
    char inst[128];                 // dominant_inst; empty: what is there stays
    bool takes_state_copy;          // the kernel serves a mlp_state_copy request
};

// Which kernel rolls the learned model out, and in what launch shape: every instantiation of kernels_mlp*.hpp is named here
// and nowhere else.  In order of precedence: the opt-in bf16 modes, the two small-network kernels, the quad kernels and
// the pipelined tile kernel of the 26-200-200-20 family, the generic kernel (spec 0..2) and its one-step form (spec 3).
MlpLaunch Engine::choose_rollout_mlp(const RolloutArgs& ra, bool per_particle_state, bool final_state, bool record) const {
    using Fn = MlpLaunch::Fn;
    const int L = mlp.n_layers;
    const unsigned tiles16 = (ra.n_pop + MLP_TP - 1) / MLP_TP, quads = (ra.n_pop + 3) / 4, rows_y = per_particle_state ? 1 : A;
    auto pick = [](Fn fn, dim3 grid, dim3 block, size_t lds, const char* name, int lds_cap = 159 * 1024) {
        MlpLaunch k;
        memset(&k, 0, sizeof(k));
        k.fn = fn; k.grid = grid; k.block = block; k.lds = lds; k.lds_cap = lds_cap; k.name = name;
        return k;
    };
    const size_t lds = (size_t)mlp_lds_layout(mlp, ra.H, U, S, mlp_nw).total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "learned-model rollout: a 16-particle tile's action block (planning_horizon x 16 x dim_u floats) plus the activation / "
            "partial-sum buffers of this network do not fit one CU's LDS (shorten the horizon or narrow the network)");
    // weights-stationary specialisations (kernels_mlp.hpp)
    int spec = 0;
    const bool small_io = mlp.tiles[0] <= 2 && mlp.tiles[L] <= 2;
    if (small_io && L == 3 && mlp.tiles[1] == mlp.tiles[2] && mlp.tiles[1] <= 16 && mlp_nw == mlp.tiles[1]) spec = 1;
    if (small_io && L == 4 && mlp.tiles[1] == mlp.tiles[2] && mlp.tiles[2] == mlp.tiles[3] && mlp.tiles[1] <= 4 && mlp_nw == mlp.tiles[1]) spec = 2;
    if (sw.mlp_generic) spec = 0;
    const bool single_step = per_particle_state && ra.H == 1;
    if (single_step) spec = 3;
    const bool ext = mlp_has_ext_act(mlp), tanh_net = mlp_is_tanh_net(mlp);

    // opt-in reduced-precision mode (kernels_mlp.hpp): never selected automatically; trajectory recording lives in
    // rollout_mlp_body's epilogue only
    if (sw.mlp_bf16 && spec == 1 && !per_particle_state && !final_state && !record) {
        const bool split = sw.mlp_bf16 == 3;
        return pick(split ? k_rollout_mlp_bf16<3> : k_rollout_mlp_bf16<1>, dim3(tiles16, A), dim3(mlp_nw * 64), lds,
                    split ? "k_rollout_mlp_bf16<3>" : "k_rollout_mlp_bf16<1>");
    }

    // small networks, one wave per four particles and nothing through LDS between layers (kernels_mlp_w4.hpp): 2..4 Dense
    // layers of at most 32 units, dim_S <= 20, dim_U <= 8 -- the reference tutorials' 4-32-32-32-3 and 26-32-32-32-20
    // (bbmpc_set_mlp packed the operands: the shape qualifies)
    if (!sw.mlp_generic && sw.mlp_w4 != 0 && !single_step && d_w4pack.p != nullptr) {
        const size_t wlds = (size_t)mlp_w4_lds_layout(ra.H, U, S).total * sizeof(float);
        if (wlds <= 159 * 1024) {
            static const Fn table[2][3] = {{k_rollout_mlp_w4<2, false>, k_rollout_mlp_w4<3, false>, k_rollout_mlp_w4<4, false>},
                                           {k_rollout_mlp_w4<2, true>, k_rollout_mlp_w4<3, true>, k_rollout_mlp_w4<4, true>}};
            static const Fn table_ext[3] = {k_rollout_mlp_w4_ext<2>, k_rollout_mlp_w4_ext<3>, k_rollout_mlp_w4_ext<4>};
            MlpLaunch k = pick(ext ? table_ext[L - 2] : table[tanh_net ? 1 : 0][L - 2], dim3((ra.n_pop + W4_TP - 1) / W4_TP, rows_y), dim3(256),
                               wlds, "k_rollout_mlp_w4");
            if (ext) snprintf(k.inst, sizeof(k.inst), "k_rollout_mlp_w4_ext<%d>", L);
            else snprintf(k.inst, sizeof(k.inst), "k_rollout_mlp_w4<%d, %s>", L, tanh_net ? "true" : "false");
            return k;
        }
    }

    // small networks: one wave per 16-particle tile, the whole Dense stack in its registers (kernels_mlp_wave.hpp)
    if (!sw.mlp_generic && sw.mlp_wave != 0 && !single_step && small_io && L >= 2 && L <= 4 && mlp.tiles[1] <= 4) {
        bool same = true;
        for (int l = 2; l < L; ++l) same = same && mlp.tiles[l] == mlp.tiles[1];
        const int wht = mlp.tiles[1];
        const size_t wlds = (size_t)mlp_wave_lds_layout(ra.H, U, S, L - 1, wht).total * sizeof(float);
        if (same && wlds <= 159 * 1024) {
            static const Fn table[2][3][4] = {
                {{k_rollout_mlp_wave<1, 1, false>, k_rollout_mlp_wave<1, 2, false>, k_rollout_mlp_wave<1, 3, false>, k_rollout_mlp_wave<1, 4, false>},
                 {k_rollout_mlp_wave<2, 1, false>, k_rollout_mlp_wave<2, 2, false>, k_rollout_mlp_wave<2, 3, false>, k_rollout_mlp_wave<2, 4, false>},
                 {k_rollout_mlp_wave<3, 1, false>, k_rollout_mlp_wave<3, 2, false>, k_rollout_mlp_wave<3, 3, false>, k_rollout_mlp_wave<3, 4, false>}},
                {{k_rollout_mlp_wave<1, 1, true>, k_rollout_mlp_wave<1, 2, true>, k_rollout_mlp_wave<1, 3, true>, k_rollout_mlp_wave<1, 4, true>},
                 {k_rollout_mlp_wave<2, 1, true>, k_rollout_mlp_wave<2, 2, true>, k_rollout_mlp_wave<2, 3, true>, k_rollout_mlp_wave<2, 4, true>},
                 {k_rollout_mlp_wave<3, 1, true>, k_rollout_mlp_wave<3, 2, true>, k_rollout_mlp_wave<3, 3, true>, k_rollout_mlp_wave<3, 4, true>}}};
            static const Fn table_ext[3][4] = {
                {k_rollout_mlp_wave<1, 1, false, true>, k_rollout_mlp_wave<1, 2, false, true>, k_rollout_mlp_wave<1, 3, false, true>, k_rollout_mlp_wave<1, 4, false, true>},
                {k_rollout_mlp_wave<2, 1, false, true>, k_rollout_mlp_wave<2, 2, false, true>, k_rollout_mlp_wave<2, 3, false, true>, k_rollout_mlp_wave<2, 4, false, true>},
                {k_rollout_mlp_wave<3, 1, false, true>, k_rollout_mlp_wave<3, 2, false, true>, k_rollout_mlp_wave<3, 3, false, true>, k_rollout_mlp_wave<3, 4, false, true>}};
            return pick(ext ? table_ext[L - 2][wht - 1] : table[tanh_net ? 1 : 0][L - 2][wht - 1], dim3(tiles16, rows_y),
                        dim3(64 * mlp_wave_waves(wht)), wlds, "k_rollout_mlp_wave");
        }
    }

    // the 26-200-200-20 tanh/tanh/linear family has its own kernels (all of them can record the trajectory)
    const bool fam_dims = spec == 1 && mlp.tiles[1] == 13 && !per_particle_state;     // (spec == 1: two hidden layers of equal tile count, <= 32 inputs and outputs)
    const bool fam_ok = fam_dims && tanh_net;
    // quad mode (4 particles per workgroup, 4x4x1_16b MFMA, all weights in registers) when the population is too
    // small to give every CU a 16-particle tile
    const bool q4_dims = mlp.dims[0] <= 28 && mlp.dims[1] == 200 && mlp.dims[2] == 200 && mlp.dims[3] <= 64;
    const bool q4_ok = fam_ok && q4_dims;
    // k_rollout_mlp_q4s: two hidden layers of 200 or of 256 units, dim_S <= 20, dim_U <= 8, any activations
    const bool wide = spec == 1 && mlp.tiles[1] == 16 && !per_particle_state && mlp.dims[0] <= 28 && mlp.dims[1] == 256 && mlp.dims[2] == 256;
    const bool q4s_ok = ((fam_dims && q4_dims) || wide) && S <= 20 && U <= 8 && mlp.dims[3] == S && d_wq4s0.p != nullptr &&
                        (ra.reward_kind == REW_CHEETAH || ra.reward_kind == REW_NONE);
    // measured on MI355X (tools/q4_sweep.py, PI2, H = 30, us per control step): a "wave" of 256 quad workgroups (one
    // per CU, 1024 particles) costs ~400 us, the 16-particle tiling ~850 us for anything up to 4096 particles:
    // quads win up to two waves (N*A <= 2048: 810 vs 860), lose from the third on (2500: 1177 vs 868)
    const long quads_total = (long)quads * A;
    bool q4 = (q4_ok || q4s_ok) && quads_total <= 512;
    if (sw.mlp_q4 >= 0) q4 = sw.mlp_q4 != 0 && (q4_ok || q4s_ok);
    // four equal waves, the state in registers, the last layer from registers, two barriers per model step (kernels_mlp_q4s.hpp)
    if (q4 && !sw.mlp_generic && sw.mlp_q4s && q4s_ok) {
        const size_t qlds = (size_t)mlp_q4s_lds_floats(wide ? 64 : 50, 7, ra.H, U) * sizeof(float);
        const int qpairs = 4 * ((ra.H * U + 3) / 4);
        if (qlds <= 160 * 1024 && qpairs <= Q4S_MAX_ACTION_PAIRS) {
            // the activations at compile time for tanh networks and, at 200 units, relu networks; at run time otherwise (RT: up
            // to sigmoid, RTX: every code).  Indexed [256 units][activations][two action pairs per thread]
            enum { F_TANH, F_RELU, F_RT, F_RTX };
            static const int codes[4][3] = {{ACT_TANH, ACT_TANH, ACT_NONE}, {ACT_RELU, ACT_RELU, ACT_NONE}, {ACT_RT, ACT_RT, ACT_RT}, {ACT_RTX, ACT_RTX, ACT_RTX}};
            static const Fn table[2][4][2] = {
                {{k_rollout_mlp_q4s<50, 7, ACT_TANH, ACT_TANH, ACT_NONE, 1>, k_rollout_mlp_q4s<50, 7, ACT_TANH, ACT_TANH, ACT_NONE, 2>},
                 {k_rollout_mlp_q4s<50, 7, ACT_RELU, ACT_RELU, ACT_NONE, 1>, k_rollout_mlp_q4s<50, 7, ACT_RELU, ACT_RELU, ACT_NONE, 2>},
                 {k_rollout_mlp_q4s<50, 7, ACT_RT, ACT_RT, ACT_RT, 1>, k_rollout_mlp_q4s<50, 7, ACT_RT, ACT_RT, ACT_RT, 2>},
                 {k_rollout_mlp_q4s<50, 7, ACT_RTX, ACT_RTX, ACT_RTX, 1>, k_rollout_mlp_q4s<50, 7, ACT_RTX, ACT_RTX, ACT_RTX, 2>}},
                {{k_rollout_mlp_q4s<64, 7, ACT_TANH, ACT_TANH, ACT_NONE, 1>, k_rollout_mlp_q4s<64, 7, ACT_TANH, ACT_TANH, ACT_NONE, 2>},
                 {nullptr, nullptr},                                                          // (no relu form at 256 units: F_RT)
                 {k_rollout_mlp_q4s<64, 7, ACT_RT, ACT_RT, ACT_RT, 1>, k_rollout_mlp_q4s<64, 7, ACT_RT, ACT_RT, ACT_RT, 2>},
                 {k_rollout_mlp_q4s<64, 7, ACT_RTX, ACT_RTX, ACT_RTX, 1>, k_rollout_mlp_q4s<64, 7, ACT_RTX, ACT_RTX, ACT_RTX, 2>}}};
            const int form = ext ? F_RTX : tanh_net ? F_TANH : (!wide && mlp_is_hidden_act_net(mlp, BBMPC_ACT_RELU)) ? F_RELU : F_RT;
            const int ne = qpairs <= 256 ? 1 : 2;
            MlpLaunch k = pick(table[wide ? 1 : 0][form][ne - 1], dim3(quads, A), dim3(256), qlds, "k_rollout_mlp_q4s", 160 * 1024);
            // the instantiation as rocprofv3 prints it (bbmpc_profile_instantiation): HG, K0G, three activations, NE
            snprintf(k.inst, sizeof(k.inst), "k_rollout_mlp_q4s<%d, 7, %d, %d, %d, %d>", wide ? 64 : 50, codes[form][0], codes[form][1],
                     codes[form][2], ne);
            k.takes_state_copy = true;
            return k;
        }
    }
    if (q4 && q4_ok && !sw.mlp_generic) {
        const size_t qlds = (size_t)mlp_q4_lds_floats(50, 7, 4, ra.H, U, S) * sizeof(float);
        if (qlds <= 160 * 1024)
            return pick(k_rollout_mlp_q4<50, 7, 4, ACT_TANH, ACT_TANH, ACT_NONE>, dim3(quads, A), dim3(256), qlds, "k_rollout_mlp_q4", 160 * 1024);
    }

    // pipelined kernel for the 26-200-200-20 family: two tiles per workgroup (software-pipelined) when tiles outnumber the
    // CUs, one tile per workgroup otherwise (more workgroups beat better per-workgroup efficiency then)
    if (fam_ok && !sw.mlp_generic) {
        const long tiles_total = (long)tiles16 * A;
        bool pair = tiles_total > 256;
        if (sw.mlp_pair >= 0) pair = sw.mlp_pair != 0;
        const int nt = pair ? 2 : 1;
        const size_t plds = (size_t)mlp_pair_lds_floats(13, ra.H, U, S, nt) * sizeof(float);
        if (plds <= 159 * 1024) {
            const bool cheetah_io = S == 20 && U == 6;
            Fn fn = k_rollout_mlp_pair<13, ACT_TANH, ACT_TANH, ACT_NONE, 1>;
            if (nt == 2 && cheetah_io && ra.H == 50 && ra.reward_kind == REW_CHEETAH && !record && mlp.half_tail[1] && mlp.half_tail[2])
                // BASELINE config 5: dimensions and the reward at compile time (no register spills, kernels_mlp.hpp)
                fn = k_rollout_mlp_pair<13, ACT_TANH, ACT_TANH, ACT_NONE, 2, 20, 6, 50, REW_CHEETAH, 1>;
            else if (nt == 2 && cheetah_io && ra.H == 50) fn = k_rollout_mlp_pair<13, ACT_TANH, ACT_TANH, ACT_NONE, 2, 20, 6, 50>;
            else if (nt == 2 && cheetah_io) fn = k_rollout_mlp_pair<13, ACT_TANH, ACT_TANH, ACT_NONE, 2, 20, 6>;
            else if (nt == 2) fn = k_rollout_mlp_pair<13, ACT_TANH, ACT_TANH, ACT_NONE, 2>;
            MlpLaunch k = pick(fn, dim3((ra.n_pop + nt * MLP_TP - 1) / (nt * MLP_TP), A), dim3(mlp_pair_waves(13, nt) * 64), plds, "k_rollout_mlp_pair");
            k.raise_lds_always = true;             // (as this branch always did)
            return k;
        }
    }

    // the generic kernel, [*_ext][spec]; the name is the caller's
    static const Fn generic[2][4] = {{k_rollout_mlp<0>, k_rollout_mlp<1>, k_rollout_mlp<2>, k_step_mlp},
                                     {k_rollout_mlp_ext<0>, k_rollout_mlp_ext<1>, k_rollout_mlp_ext<2>, k_step_mlp_ext}};
    return pick(generic[ext ? 1 : 0][spec], dim3(tiles16, rows_y), dim3(mlp_nw * 64), lds, nullptr);
}

void Engine::launch_rollout_mlp(int mode, bool pen, RolloutArgs& ra, bool per_particle_state, float* final_state, float* traj_out) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    const MlpLaunch k = choose_rollout_mlp(ra, per_particle_state, final_state != nullptr, traj_out != nullptr);
    MlpRolloutArgs q;
    memset(&q, 0, sizeof(q));
    q.r = ra;
    q.m = mlp;
    q.mode = mode;
    q.pen = pen ? 1 : 0;
    q.per_particle_state = per_particle_state ? 1 : 0;
    q.final_state = final_state;
    q.nw = mlp_nw;
    q.traj = traj_out;
    for (int l = 0; l < mlp.n_layers; ++l) { q.wraw[l] = d_wraw[l].p; q.braw[l] = d_braw[l].p; q.wq4[l] = d_wq4[l].p; q.wp4[l] = d_wpack4[l].p; q.wbf[l] = reinterpret_cast<const uint4*>(d_wbf[l].p); }
    q.wq4s0 = d_wq4s0.p;
    q.w4pack = d_w4pack.p;
    if (k.takes_state_copy) {
        q.state_copy = mlp_state_copy;
        mlp_state_copy = nullptr;
    }
    if (k.raise_lds_always || k.lds > 64 * 1024) ensure_max_lds((const void*)k.fn, k.lds_cap);
    if (k.name) dominant_kernel = k.name;
    if (k.inst[0]) memcpy(dominant_inst, k.inst, sizeof(dominant_inst));
    prof_begin();
    hipLaunchKernelGGL(k.fn, k.grid, k.block, k.lds, stream, q);
    HIP_CHECK(hipGetLastError());
    prof_end();
}

// bbmpc_predict_trajectories on a learned model with a built-in reward: one launch of k_traj_mlp (kernels_mlp_traj.hpp),
// 16 rows per workgroup whatever the network -- the generic kernel's coverage (<= 8 layers, width <= 512)
void Engine::traj_mlp(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    MlpTrajArgs q;
    memset(&q, 0, sizeof(q));
    q.m = mlp;
    for (int l = 0; l < mlp.n_layers; ++l) q.wp4[l] = d_wpack4[l].p;
    q.nw = mlp_nw;
    q.B = batch; q.Hq = horizon; q.S = S; q.U = U;
    q.reward_kind = builtin_reward_kind();
    q.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER) ? 1 : 0;
    q.states = d_states;
    q.seq = d_seq;
    q.states_out = d_states_out;
    q.rewards_out = d_rewards_out;
    const size_t lds = (size_t)mlp_traj_lds_layout(mlp, U, S, mlp_nw).total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED, "trajectory prediction: the activation / partial-sum buffers of this network do not fit one CU's LDS");
    launch_args(mlp_has_ext_act(mlp) ? k_traj_mlp<true> : k_traj_mlp<false>, dim3((batch + MLP_TP - 1) / MLP_TP), dim3(mlp_nw * 64), lds, stream, q);
}

// What the six argument structs of the particle frames (kernels_mlp_particles.hpp, kernels_mlp_traj_particles.hpp) share:
// the model's operands or the ensemble's with their member strides, the log-variance heads, and for kind MLP_PART_GAUSS the
// LDS of the doubled last layer in `lds`
template <class ARGS, class PA>
static void mlp_particle_operands(const Engine& e, const PA& pa, ARGS& q, size_t& lds) {
    const MlpDesc& m = e.mlp;
    const bool ens = e.ens_E > 0;
    memset(&q, 0, sizeof(q));
    q.m = m;
    q.nw = e.mlp_nw;
    q.p = pa;
    for (int l = 0; l < m.n_layers; ++l) {
        q.wp4[l] = ens ? e.d_ens_wp4[l].p : e.d_wpack4[l].p;
        q.m.bpack[l] = ens ? e.d_ens_bp[l].p : e.d_bpack[l].p;
        if constexpr (ARGS::KIND != MLP_PART_PLAIN) {
            q.wstride[l] = ens ? m.tiles[l + 1] * m.tiles[l] * 256 : 0;
            q.bstride[l] = ens ? m.tiles[l + 1] * 256 : 0;
        }
    }
    if constexpr (ARGS::KIND != MLP_PART_PLAIN) q.E = std::max(1, e.ens_E);
    if constexpr (ARGS::KIND == MLP_PART_GAUSS) {
        const int Ll = m.n_layers - 1;
        q.hp4 = e.d_lv_wp4.p;
        q.hbp = e.d_lv_bp.p;
        q.hwstride = m.tiles[Ll + 1] * m.tiles[Ll] * 256;
        q.hbstride = m.tiles[Ll + 1] * 256;
        q.min_logvar = e.d_lv_bounds.p;
        q.max_logvar = e.d_lv_bounds.p + e.S;
        lds = (size_t)mlp_gauss_lds_layout(m, e.U, e.S, e.mlp_nw).total * sizeof(float);
        REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED, "particle rollout: the log-variance head's partial sums do not fit one CU's LDS");
    }
}

// Particle rollouts of a learned model (bbmpc_set_particles; built-in reward, or with pa.traj the TRAJ form for a HIP-source one): one launch of the frame of
// kernels_mlp_particles.hpp, 16 (candidate, particle) rows per workgroup, grid.y = agent -- the coverage of k_traj_mlp,
// always fp32.  Kind MLP_PART_PLAIN; with an ensemble installed (bbmpc_set_mlp_ensemble) MLP_PART_ENS, rows grouped by
// member and grid.z = member; with log-variance heads (bbmpc_set_mlp_logvar_head), with or without an ensemble,
// MLP_PART_GAUSS (without an ensemble one "member", the primary's operands at stride 0)
void Engine::launch_rollout_mlp_particles(const ParticleArgs& pa) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    size_t lds = (size_t)mlp_traj_lds_layout(mlp, U, S, mlp_nw).total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED, "particle rollout: the activation / partial-sum buffers of this network do not fit one CU's LDS");
    // (the kernel addresses its action source and the noise with 32-bit offsets)
    const long act_elems = pa.from_ref ? (long)pa.n_pop * A * pa.HU : (long)A * pa.HU * pa.Nst;
    REQUIRE(act_elems < (1L << 31) && (long)A * pa.P * pa.H * S < (1L << 31), BBMPC_E_UNSUPPORTED,
            "particle rollout: more than 2^31 action or noise elements per launch");
    if (pa.traj)
        REQUIRE((long)pa.H * A * S * pa.RS < (1L << 31), BBMPC_E_UNSUPPORTED, "particle rollout: more than 2^31 trajectory elements per launch");
    const int kind = lv_heads > 0 ? MLP_PART_GAUSS : ens_E > 0 ? MLP_PART_ENS : MLP_PART_PLAIN;
    const int E = std::max(1, ens_E);
    if (kind == MLP_PART_GAUSS) REQUIRE(lv_heads == E && pa.P % E == 0, BBMPC_E_INVALID, "internal: log-variance heads per model");
    if (kind == MLP_PART_ENS) REQUIRE(pa.P % E == 0, BBMPC_E_INVALID, "internal: particles per ensemble member");
    const long rows = (long)pa.n_pop * (pa.P / E);            // per (agent, member)
    dim3 grid((unsigned)((rows + MLP_TP - 1) / MLP_TP), A, E), block(mlp_nw * 64);
    const bool ext = mlp_has_ext_act(mlp);
    // the arguments of kind ARGS::KIND and its launch; pa.traj set (a HIP-source reward): the TRAJ form, which stores every noisy
    // next state and leaves the returns to the scorer (its row slots lie behind the layout)
    auto launch = [&](auto q) {
        using ARGS = decltype(q);
        mlp_particle_operands(*this, pa, q, lds);
        const size_t slots = MLP_PART_ROWSLOT * sizeof(int);
        if (pa.traj)
            launch_args(ext ? k_rollout_mlp_particles_kind<ARGS, true, true> : k_rollout_mlp_particles_kind<ARGS, false, true>, grid, block,
                        lds + slots, stream, q, 159 * 1024 + (int)slots);
        else
            launch_args(ext ? k_rollout_mlp_particles_kind<ARGS, true, false> : k_rollout_mlp_particles_kind<ARGS, false, false>, grid, block,
                        lds, stream, q);
    };
    if (kind == MLP_PART_GAUSS) launch(MlpGaussParticleArgs());
    else if (kind == MLP_PART_ENS) launch(MlpEnsParticleArgs());
    else launch(MlpParticleArgs());
}

// bbmpc_predict_trajectory_particles on a learned model with a built-in reward: one launch of the frame of
// kernels_mlp_traj_particles.hpp, 16 (b, p) rows per workgroup, grid.z = member; the kinds, operands and LDS limits of
// launch_rollout_mlp_particles above
void Engine::launch_traj_mlp_particles(const TrajParticleArgs& pa) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    size_t lds = (size_t)mlp_traj_lds_layout(mlp, U, S, mlp_nw).total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED, "particle rollout: the activation / partial-sum buffers of this network do not fit one CU's LDS");
    const int kind = lv_heads > 0 ? MLP_PART_GAUSS : ens_E > 0 ? MLP_PART_ENS : MLP_PART_PLAIN;
    const int E = std::max(1, ens_E);
    if (kind == MLP_PART_GAUSS) REQUIRE(lv_heads == E && pa.P % E == 0, BBMPC_E_INVALID, "internal: log-variance heads per model");
    if (kind == MLP_PART_ENS) REQUIRE(pa.P % E == 0, BBMPC_E_INVALID, "internal: particles per ensemble member");
    const long rows = (long)pa.B * (pa.P / E);                // per member
    dim3 grid((unsigned)((rows + MLP_TP - 1) / MLP_TP), 1, E), block(mlp_nw * 64);
    const bool ext = mlp_has_ext_act(mlp);
    auto launch = [&](auto q) {
        using ARGS = decltype(q);
        mlp_particle_operands(*this, pa, q, lds);
        const size_t rowmap = MLP_TRAJ_PART_ROWMAP * sizeof(int);                 // (the row map of the tile lies behind the layout)
        launch_args(ext ? k_traj_mlp_particles_kind<ARGS, true> : k_traj_mlp_particles_kind<ARGS, false>, grid, block, lds + rowmap, stream, q,
                    159 * 1024 + (int)rowmap);
    };
    if (kind == MLP_PART_GAUSS) launch(MlpGaussTrajParticleArgs());
    else if (kind == MLP_PART_ENS) launch(MlpEnsTrajParticleArgs());
    else launch(MlpTrajParticleArgs());
}

// ------------------------------------------------------------------------------------------------
// learned reward model (bbmpc_set_reward_mlp; kernels_reward_mlp.hpp)
// ------------------------------------------------------------------------------------------------
// What the two setters of a one-output Dense stack share (the reward model here, the terminal value below): the
// descriptor's shape and the packed operands on the host, then the uploads.
struct DenseStackHost {
    RewMlpDesc d;
    std::vector<float> w4[MLP_MAX_LAYERS], bp[MLP_MAX_LAYERS];
};

// The argument checks of the Dense-stack setters (reward model, terminal value, policy prior), in the order each of them has
// always made them: pointers and layer count, own_first(), widths, own_shape() -- what the setter asks of dims[0] and
// dims[n_layers] --, then every layer's activation and pointers and the n_stats statistics vectors.
template <class OwnFirst, class OwnShape>
static void check_dense_stack(const std::string& prefix, const char* too_few_layers, int n_layers, const int32_t* dims, const int32_t* acts,
                              const float* const* w, const float* const* b, int is_normalized, const float* const* stats, int n_stats,
                              OwnFirst own_first, OwnShape own_shape) {
    REQUIRE(dims && acts && w && b, BBMPC_E_INVALID, "null argument");
    REQUIRE(n_layers >= 1, BBMPC_E_INVALID, prefix + too_few_layers);
    REQUIRE(n_layers <= MLP_MAX_LAYERS, BBMPC_E_UNSUPPORTED, prefix + "1..8 Dense layers are supported");
    own_first();
    for (int l = 0; l <= n_layers; ++l) REQUIRE(dims[l] >= 1, BBMPC_E_INVALID, "layer width must be >= 1");
    own_shape();
    for (int l = 0; l < n_layers; ++l) {
        REQUIRE(acts[l] >= BBMPC_ACT_NONE && acts[l] <= BBMPC_ACT_RELU6, BBMPC_E_INVALID, "unknown activation");
        REQUIRE(w[l] && b[l], BBMPC_E_INVALID, "null weight/bias pointer");
    }
    if (is_normalized) {
        REQUIRE(stats, BBMPC_E_INVALID, "normalisation statistics are required when is_normalized != 0");
        for (int i = 0; i < n_stats; ++i) REQUIRE(stats[i], BBMPC_E_INVALID, "null statistics vector");
    }
}

// Widths and tiles of a Dense stack, features in index order (what mlp_pack_layer reads) -> the waves of a workgroup
static int dense_stack_shape(MlpDesc& shape, int n_layers, const int32_t* dims) {
    memset(&shape, 0, sizeof(shape));
    shape.n_layers = n_layers;
    int hidden_tiles = 1;
    for (int l = 0; l <= n_layers; ++l) {
        shape.dims[l] = dims[l];
        shape.tiles[l] = (dims[l] + 15) / 16;
        if (l >= 1 && l < n_layers) hidden_tiles = std::max(hidden_tiles, shape.tiles[l]);
    }
    return std::min(16, hidden_tiles);
}

static void dense_stack_pack(DenseStackHost& hs, int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w,
                             const float* const* b, int input_mask, int S, int U) {
    RewMlpDesc& d = hs.d;
    memset(&d, 0, sizeof(d));
    MlpDesc shape;
    d.nw = dense_stack_shape(shape, n_layers, dims);
    d.n_layers = n_layers;
    for (int l = 0; l <= n_layers; ++l) {
        d.dims[l] = shape.dims[l];
        d.tiles[l] = shape.tiles[l];
    }
    d.mask = input_mask; d.S = S; d.U = U; d.D = dims[0];
    d.off_a = (input_mask & 1) ? S : 0;
    d.off_n = d.off_a + ((input_mask & 2) ? U : 0);
    for (int l = 0; l < n_layers; ++l) {
        d.act[l] = acts[l];
        if (l < n_layers - 1) {
            std::vector<float> wp;
            mlp_pack_layer(shape, l, w[l], b[l], wp, hs.w4[l], hs.bp[l]);
        }
    }
}

static void dense_stack_upload(DenseStackHost& hs, const float* const* w, const float* const* b, int is_normalized, const float* const* stats,
                               DevBuf<float>* d_wp4, DevBuf<float>* d_bp, DevBuf<float>& d_last, DevBuf<float>& d_stats) {
    RewMlpDesc& d = hs.d;
    const int n_layers = d.n_layers, D = d.D;
    for (int l = 0; l < n_layers - 1; ++l) {
        upload(d_wp4[l], hs.w4[l]);
        upload(d_bp[l], hs.bp[l]);
        d.wp4[l] = d_wp4[l].p;
        d.bpack[l] = d_bp[l].p;
    }
    upload(d_last, std::vector<float>(w[n_layers - 1], w[n_layers - 1] + d.dims[n_layers - 1]));      // [K][1]
    d.wlast = d_last.p;
    d.blast = b[n_layers - 1][0];
    d.normalized = is_normalized ? 1 : 0;
    if (is_normalized) {
        std::vector<float> st(stats[0], stats[0] + D);
        st.insert(st.end(), stats[1], stats[1] + D);
        upload(d_stats, st);
        d.mean_in = d_stats.p;
        d.std_in = d_stats.p + D;
        d.mean_r = stats[2][0];
        d.std_r = stats[3][0];
    }
}

// Everything is checked and packed on the host before the handle is touched, so a refusal leaves it as it was.
void Engine::set_reward_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                            int input_mask, int is_normalized, const float* const* stats) {
    REQUIRE(cfg.reward == BBMPC_REW_MLP, BBMPC_E_STATE, "handle was not created with BBMPC_REW_MLP");
    const int D = ((input_mask & 1) ? S : 0) + ((input_mask & 2) ? U : 0) + ((input_mask & 4) ? S : 0);
    check_dense_stack(
        "reward model: ", "at least one Dense layer", n_layers, dims, acts, w, b, is_normalized, stats, 4,
        [&] { REQUIRE(input_mask >= 1 && input_mask <= 7, BBMPC_E_INVALID, "reward model: input_mask must select at least one of s_t (1), a_t (2), s_t+1 (4)"); },
        [&] {
            REQUIRE(dims[0] == D, BBMPC_E_INVALID,
                    "reward model: dims[0] = " + std::to_string(dims[0]) + " but input_mask selects " + std::to_string(D) + " input columns");
            REQUIRE(dims[n_layers] == 1, BBMPC_E_INVALID, "reward model: the last layer must have one output (dims[n_layers] == 1)");
        });
    REQUIRE(D <= REW_MLP_MAX_IN, BBMPC_E_UNSUPPORTED, "reward model: more than 192 input columns");
    for (int l = 1; l < n_layers; ++l) REQUIRE(dims[l] <= REW_MLP_MAX_HIDDEN, BBMPC_E_UNSUPPORTED, "hidden width > 512 not supported");
    DenseStackHost hs;
    dense_stack_pack(hs, n_layers, dims, acts, w, b, input_mask, S, U);
    REQUIRE((size_t)rew_mlp_lds_layout(hs.d).total * sizeof(float) <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "reward model: the activation buffers of this network do not fit one CU's LDS");
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));
    rew_mlp_ready = false;
    dense_stack_upload(hs, w, b, is_normalized, stats, d_rw_wp4, d_rw_bp, d_rw_last, d_rw_stats);
    rew_mlp = hs.d;
    rew_mlp_ready = true;
    pg_host[1].keep(n_layers, dims, acts, w, b);        // (plan gradients pack W^T from these at their next call)
    pg_stale[1] = true;
}

// ------------------------------------------------------------------------------------------------
// learned terminal value (bbmpc_set_terminal_value_mlp; kernels_reward_mlp.hpp)
// ------------------------------------------------------------------------------------------------
// As set_reward_mlp: checked and packed on the host before the handle is touched.  n_layers = 0 removes the network.
void Engine::set_terminal_value_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                                    int is_normalized, const float* const* stats, float terminal_weight) {
    if (n_layers == 0) {                        // back to the routing the handle had: nothing else of it was ever changed
        if (!val_mlp_ready) return;
        invalidate_step_graph();
        HIP_CHECK(hipStreamSynchronize(stream));
        val_mlp_ready = false;
        return;
    }
    check_dense_stack("terminal value: ", "n_layers must be >= 0", n_layers, dims, acts, w, b, is_normalized, stats, 4, [] {}, [&] {
        REQUIRE(dims[0] == S, BBMPC_E_INVALID,
                "terminal value: dims[0] = " + std::to_string(dims[0]) + " but the network reads the state, dim_s = " + std::to_string(S));
        REQUIRE(dims[n_layers] == 1, BBMPC_E_INVALID, "terminal value: the last layer must have one output (dims[n_layers] == 1)");
    });
    REQUIRE(std::isfinite(terminal_weight), BBMPC_E_INVALID, "terminal value: terminal_weight must be finite");
    for (int l = 1; l < n_layers; ++l) REQUIRE(dims[l] <= REW_MLP_MAX_HIDDEN, BBMPC_E_UNSUPPORTED, "hidden width > 512 not supported");
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_UNSUPPORTED,
            "a learned terminal value closes the rollouts of a learned model: the handle needs BBMPC_DYN_MLP, not analytic or user dynamics");
    REQUIRE(!user_callbacks(), BBMPC_E_UNSUPPORTED,
            "a learned terminal value beside a callback plug-in: the step-wise rollout has no terminal-value form (use a HIP-source reward)");
    REQUIRE(!has_xform(), BBMPC_E_UNSUPPORTED,
            "a learned terminal value beside an inverse target transform: the transform rollout has no terminal-value form");
    REQUIRE(!particles_on(), BBMPC_E_UNSUPPORTED,
            "a learned terminal value with particles on: the particle evaluator has no terminal term (bbmpc_set_particles(0) first)");
    DenseStackHost hs;
    dense_stack_pack(hs, n_layers, dims, acts, w, b, 1, S, U);
    REQUIRE((size_t)rew_mlp_lds_layout(hs.d).total * sizeof(float) <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "terminal value: the activation buffers of this network do not fit one CU's LDS");
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));
    val_mlp_ready = false;
    dense_stack_upload(hs, w, b, is_normalized, stats, d_vl_wp4, d_vl_bp, d_vl_last, d_vl_stats);
    val_mlp = hs.d;
    val_weight = terminal_weight;
    val_mlp_ready = true;
    pg_host[2].keep(n_layers, dims, acts, w, b);
    pg_stale[2] = true;
}

// Whatever the handle runs today for its reward kind, with u_traj recording on, then the terminal term in one launch.
// Built-in rewards: every learned-model kernel family records beside a run-time reward (launch_rollout_mlp keeps the
// compile-time-reward pair kernel and the opt-in bf16 kernel, which do not, for calls without a trajectory pointer).
void Engine::rollout_terminal_value(int mode, bool pen, RolloutArgs& ra) {
    if (cfg.reward == BBMPC_REW_MLP) {
        rollout_mlp_reward_mlp(mode, pen, ra);
    } else if (cfg.reward == BBMPC_REW_USER) {            // HIP source (callbacks were refused); BBMPC_USER_STEPWISE has no recording form
        rollout_mlp_user_reward(mode, pen, ra);
    } else {
        const size_t need = (size_t)ra.H * A * ra.Nst * S;
        if (u_traj.n < need) u_traj.alloc(need);
        launch_rollout_mlp(mode, pen, ra, false, nullptr, u_traj.p);
    }
    ValMlpTermArgs q;
    memset(&q, 0, sizeof(q));
    q.m = val_mlp;
    q.n_pop = ra.n_pop; q.A = A; q.Nst = ra.Nst;
    q.weight = val_weight;
    q.last = u_traj.p + (size_t)(ra.H - 1) * A * ra.Nst * S;
    q.rewards = ra.rewards;
    const size_t lds = (size_t)rew_mlp_lds_layout(val_mlp).total * sizeof(float);
    launch_args(k_value_mlp_terminal, dim3((ra.n_pop + MLP_TP - 1) / MLP_TP, A), dim3(val_mlp.nw * 64), lds, stream, q);
}

// V on B rows of states [B][S]: the rows frame with the value network's descriptor, no weight and no NaN rule
void Engine::terminal_value_rows(const float* d_states, int batch, float* d_out) {
    REQUIRE(val_mlp_ready, BBMPC_E_STATE, "terminal value: call bbmpc_set_terminal_value_mlp before computing");
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    RewMlpRowsArgs q;
    memset(&q, 0, sizeof(q));
    q.m = val_mlp;
    q.B = batch;
    q.cur = d_states; q.cur_stride = S;
    q.act = d_states; q.nxt = d_states;                   // never read: the mask selects s_t alone
    q.out = d_out;
    const size_t lds = (size_t)rew_mlp_lds_layout(val_mlp).total * sizeof(float);
    launch_args(k_reward_mlp_rows, dim3((batch + MLP_TP - 1) / MLP_TP), dim3(val_mlp.nw * 64), lds, stream, q);
}

// ------------------------------------------------------------------------------------------------
// discounted, termination-aware returns (bbmpc_set_return_shaping; kernels_return_shaping.hpp)
// ------------------------------------------------------------------------------------------------
// Everything is checked before the handle is touched, so a refusal leaves it as it was.  discount == 1 with both bounds
// NULL switches shaping off: the handle's routing and scores are then what they were before it was ever set.
void Engine::set_return_shaping(float discount, const float* state_lo, const float* state_hi, float terminal_reward) {
    REQUIRE(std::isfinite(discount) && discount > 0.0f && discount <= 1.0f, BBMPC_E_INVALID, "return shaping: discount must be in (0, 1]");
    REQUIRE(std::isfinite(terminal_reward), BBMPC_E_INVALID, "return shaping: terminal_reward must be finite");
    for (int i = 0; i < S; ++i) {
        const float l = state_lo ? state_lo[i] : -INFINITY, h = state_hi ? state_hi[i] : INFINITY;
        REQUIRE(l == l && h == h, BBMPC_E_INVALID, "return shaping: state bound " + std::to_string(i) + " is NaN (use -inf / +inf for unbounded)");
        REQUIRE(l <= h, BBMPC_E_INVALID, "return shaping: state_lo[" + std::to_string(i) + "] exceeds state_hi[" + std::to_string(i) + "]");
    }
    if (discount == 1.0f && !state_lo && !state_hi) {
        if (!sh_on) return;
        invalidate_step_graph();
        HIP_CHECK(hipStreamSynchronize(stream));
        sh_on = false;
        sh_last_npop = sh_last_Nst = 0;
        return;
    }
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_UNSUPPORTED,
            "return shaping walks the recorded rollouts of a learned model: the handle needs BBMPC_DYN_MLP, not analytic or user dynamics");
    REQUIRE(cfg.reward != BBMPC_REW_USER, BBMPC_E_UNSUPPORTED,
            "return shaping beside a BBMPC_REW_USER reward (HIP source or callback): its step rewards are summed inside run-time compiled "
            "code; use a built-in reward or BBMPC_REW_MLP");
    REQUIRE(!has_xform(), BBMPC_E_UNSUPPORTED,
            "return shaping beside an inverse target transform (bbmpc_set_inverse_transform_source): the transform rollout has no shaped form");
    REQUIRE(!particles_on(), BBMPC_E_UNSUPPORTED,
            "return shaping with particles on (bbmpc_set_particles): the particle evaluator has no shaped form (bbmpc_set_particles(0) first)");
    REQUIRE(!grad_on(), BBMPC_E_UNSUPPORTED,
            "return shaping beside gradient refinement (bbmpc_set_grad_refine): the gradient steps climb the unshaped return; switch it "
            "off first (steps = 0)");
    std::vector<float> box((size_t)2 * S);
    for (int i = 0; i < S; ++i) {
        box[i] = state_lo ? state_lo[i] : -INFINITY;
        box[S + i] = state_hi ? state_hi[i] : INFINITY;
    }
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));               // (nothing in flight reads the box that is replaced)
    sh_on = false;
    upload(d_sh_box, box);
    sh_gamma = discount;
    sh_term_reward = terminal_reward;
    sh_last_npop = sh_last_Nst = 0;
    sh_on = true;
}

// The launch sequences of a shaping handle.  A built-in reward: the rollout with reward kind REW_NONE and recording on, the
// way rollout_mlp_user_reward runs it -- k_shaped_return recomputes the step rewards with reward_generic.  BBMPC_REW_MLP:
// the rollout and k_reward_mlp_traj, whose step buffer k_shaped_return reads in k_reward_mlp_finish's place.  A value
// network: one k_reward_mlp_rows launch over the last plane (k_value_mlp_terminal's + w * V is unconditional).
void Engine::rollout_shaped(int mode, bool pen, RolloutArgs& ra) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    REQUIRE((long)ra.H * A * ra.Nst * S < (1L << 31), BBMPC_E_UNSUPPORTED, "return shaping: more than 2^31 trajectory elements per launch");
    const size_t need = (size_t)ra.H * A * ra.Nst * S, need_n = (size_t)A * ra.Nst;
    if (u_traj.n < need) u_traj.alloc(need);
    if (d_sh_tsteps.n < need_n) d_sh_tsteps.alloc(need_n);
    if (value_on() && d_sh_vterm.n < need_n) d_sh_vterm.alloc(need_n);
    const bool learned = cfg.reward == BBMPC_REW_MLP;
    if (learned) {
        rollout_mlp_reward_mlp(mode, pen, ra, false);
    } else {
        struct Restore { int& kind; int was; ~Restore() { kind = was; } } restore{ra.reward_kind, ra.reward_kind};
        ra.reward_kind = REW_NONE;                        // leaves -(penalty) in ra.rewards
        launch_rollout_mlp(mode, pen, ra, false, nullptr, u_traj.p);
    }
    if (value_on()) {                                     // V of the last plane: per agent its n_pop rows, the padding rows stay untouched
        const size_t vlds = (size_t)rew_mlp_lds_layout(val_mlp).total * sizeof(float);
        for (int a = 0; a < A; ++a) {
            RewMlpRowsArgs r;
            memset(&r, 0, sizeof(r));
            r.m = val_mlp;
            r.B = ra.n_pop;
            r.cur = u_traj.p + ((size_t)(ra.H - 1) * A + a) * ra.Nst * S; r.cur_stride = S;
            r.act = r.cur; r.nxt = r.cur;                 // never read: the mask selects s_t alone
            r.out = d_sh_vterm.p + (size_t)a * ra.Nst;
            launch_args(k_reward_mlp_rows, dim3((r.B + MLP_TP - 1) / MLP_TP), dim3(val_mlp.nw * 64), vlds, stream, r);
        }
    }
    ShapedReturnArgs q;
    memset(&q, 0, sizeof(q));
    q.n_pop = ra.n_pop; q.A = A; q.H = ra.H; q.Nst = ra.Nst; q.HU = ra.HU; q.S = S; q.U = U;
    q.from_ref = mode == SRC_REF ? 1 : 0;
    q.reward_kind = learned ? REW_NONE : (int)cfg.reward;
    q.fix_q1 = fix(BBMPC_FIX_Q1_REWARD_ARG_ORDER) ? 1 : 0;
    q.gamma = sh_gamma; q.term_reward = sh_term_reward; q.weight = val_weight;
    q.state = ra.state;
    q.traj = u_traj.p;
    q.seq = ra.seq;
    q.cand = mode == SRC_BUF ? ra.cand : ra.samples;
    if (mode != SRC_REF) REQUIRE(q.cand, BBMPC_E_STATE, "return shaping over the learned model: no candidate buffer");
    // a rollout that clips (pen) must have written the clipped candidates back: they are the a_t of the rule
    if (mode == SRC_BUF && pen) REQUIRE(ra.samples == ra.cand, BBMPC_E_INVALID, "internal: return shaping needs the clipped candidates written back");
    q.step = learned ? d_rw_step.p : nullptr;
    q.vterm = value_on() ? d_sh_vterm.p : nullptr;
    q.box = d_sh_box.p;
    q.rewards = ra.rewards;
    q.tsteps = d_sh_tsteps.p;
    const size_t lds = (size_t)shaped_return_lds_floats(S, U) * sizeof(float);
    const dim3 grid((ra.n_pop + SHAPED_LANES - 1) / SHAPED_LANES, A), block(SHAPED_LANES);
    if (S % 4 == 0) hipLaunchKernelGGL(k_shaped_return<true>, grid, block, lds, stream, q);
    else hipLaunchKernelGGL(k_shaped_return<false>, grid, block, lds, stream, q);
    HIP_CHECK(hipGetLastError());
    sh_last_npop = ra.n_pop;
    sh_last_Nst = ra.Nst;
}

// T of the most recent rollout, [A][n_pop]
void Engine::termination_steps(int32_t* out, int n) {
    REQUIRE(shaping_on(), BBMPC_E_STATE, "termination steps: return shaping is off (bbmpc_set_return_shaping)");
    REQUIRE(sh_last_npop > 0, BBMPC_E_STATE, "termination steps: nothing has been rolled out since return shaping was set");
    REQUIRE(n == A * sh_last_npop, BBMPC_E_INVALID,
            "termination steps: n must be num_agents * (candidates of the most recent rollout) = " + std::to_string(A * sh_last_npop));
    HIP_CHECK(hipMemcpy2DAsync(out, (size_t)sh_last_npop * 4, d_sh_tsteps.p, (size_t)sh_last_Nst * 4, (size_t)sh_last_npop * 4, A,
                               hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
}

// The learned model's rollout with a learned reward: Engine::rollout_mlp_user_reward's sequence with the network in place
// of the user's function -- the MFMA rollout (reward kind REW_NONE) records u_traj and leaves -(penalty) in ra.rewards,
// k_reward_mlp_traj scores every (candidate, step) row, k_reward_mlp_finish sums the steps.
void Engine::rollout_mlp_reward_mlp(int mode, bool pen, RolloutArgs& ra, bool finish) {
    REQUIRE(rew_mlp_ready, BBMPC_E_STATE, "learned reward: call bbmpc_set_reward_mlp before computing");
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    const size_t need = (size_t)ra.H * A * ra.Nst * S, need_r = (size_t)ra.H * A * ra.Nst;
    if (u_traj.n < need) u_traj.alloc(need);
    if (d_rw_step.n < need_r) d_rw_step.alloc(need_r);
    {   // BBMPC_PROF_REWARD_MLP: the profiling events go around the scorer below, not around the rollout kernel
        struct Restore { bool& flag; bool was; ~Restore() { flag = was; } } restore{profiling, profiling};
        if (sw.prof_reward_mlp) profiling = false;
        launch_rollout_mlp(mode, pen, ra, false, nullptr, u_traj.p);
    }
    RewMlpTrajArgs q;
    memset(&q, 0, sizeof(q));
    q.m = rew_mlp;
    q.n_pop = ra.n_pop; q.A = A; q.H = ra.H; q.Nst = ra.Nst; q.HU = ra.HU;
    q.from_ref = mode == SRC_REF ? 1 : 0;
    q.state = ra.state;
    q.traj = u_traj.p;
    q.seq = ra.seq;
    q.cand = mode == SRC_BUF ? ra.cand : ra.samples;
    q.step_out = d_rw_step.p;
    if (mode != SRC_REF) REQUIRE(q.cand, BBMPC_E_STATE, "learned reward over the learned model: no candidate buffer");
    // steps are independent rows: enough t-chunks that two rounds of workgroups cover the CUs even when the population is a
    // few tiles (the number of agents plays no part, and the chunking none in the result: the steps are summed afterwards)
    const int tiles = (ra.n_pop + MLP_TP - 1) / MLP_TP;
    const int chunks = std::max(1, std::min(ra.H, (512 + tiles - 1) / tiles));
    q.tchunk = (ra.H + chunks - 1) / chunks;
    const size_t lds = (size_t)rew_mlp_lds_layout(rew_mlp).total * sizeof(float);
    if (lds > 64 * 1024) ensure_max_lds((const void*)k_reward_mlp_traj, 159 * 1024);       // (in front of the profiling event)
    dim3 grid(tiles, A, (ra.H + q.tchunk - 1) / q.tchunk), block(rew_mlp.nw * 64);
    if (sw.prof_reward_mlp) {
        dominant_kernel = "k_reward_mlp_traj";
        prof_begin();
    }
    hipLaunchKernelGGL(k_reward_mlp_traj, grid, block, lds, stream, q);
    if (sw.prof_reward_mlp) prof_end();
    if (finish)                                           // (return shaping walks the steps itself: Engine::rollout_shaped)
        hipLaunchKernelGGL(k_reward_mlp_finish, dim3((ra.n_pop + 255) / 256, A), dim3(256), 0, stream, ra.n_pop, A, ra.H, ra.Nst,
                           (const float*)d_rw_step.p, ra.rewards);
    HIP_CHECK(hipGetLastError());
}

void Engine::reward_mlp_rows(const RewMlpRowsArgs& rows) {
    REQUIRE(rew_mlp_ready, BBMPC_E_STATE, "learned reward: call bbmpc_set_reward_mlp before computing");
    RewMlpRowsArgs q = rows;
    q.m = rew_mlp;
    const size_t lds = (size_t)rew_mlp_lds_layout(rew_mlp).total * sizeof(float);
    launch_args(k_reward_mlp_rows, dim3((q.B + MLP_TP - 1) / MLP_TP), dim3(rew_mlp.nw * 64), lds, stream, q);
}

// bbmpc_predict_trajectories with a learned reward: the states from k_traj_mlp (they do not depend on the reward), then ONE
// launch of the rows frame over the B * Hq (row, step) pairs of states_out [B, Hq, S]
void Engine::traj_mlp_reward_mlp(const float* d_states, const float* d_seq, int batch, int horizon, float* d_states_out, float* d_rewards_out) {
    REQUIRE(rew_mlp_ready, BBMPC_E_STATE, "learned reward: call bbmpc_set_reward_mlp before computing");
    REQUIRE((long)batch * horizon < (1L << 31), BBMPC_E_UNSUPPORTED, "trajectory prediction with a learned reward: more than 2^31 (row, step) pairs");
    float* so = d_states_out;
    if (!so) {
        const size_t ns = (size_t)batch * horizon * S;
        if (d_rw_states.n < ns) d_rw_states.alloc(ns);
        so = d_rw_states.p;
    }
    traj_mlp(d_states, d_seq, batch, horizon, so, nullptr);
    RewMlpRowsArgs q;
    memset(&q, 0, sizeof(q));
    q.B = batch * horizon;
    q.period = horizon; q.cur_shift = 1;
    q.first = d_states;
    q.cur = so; q.cur_stride = S;
    q.act = d_seq; q.act_stride = U;
    q.nxt = so; q.nxt_stride = S;
    q.out = d_rewards_out;
    reward_mlp_rows(q);
}

// ------------------------------------------------------------------------------------------------
// learned policy prior (bbmpc_set_policy_prior_mlp; kernels_policy_prior.hpp)
// ------------------------------------------------------------------------------------------------
// Everything is checked and packed on the host before the handle is touched, so a refusal leaves it as it was.
// n_layers = 0 removes the network.
void Engine::set_policy_prior_mlp(int n_layers, const int32_t* dims, const int32_t* acts, const float* const* w, const float* const* b,
                                  int is_normalized, const float* const* stats, int count, float noise_std) {
    if (n_layers == 0) {                        // back to the routing the handle had: nothing else of it was ever changed
        if (!prior_ready) return;
        invalidate_step_graph();
        HIP_CHECK(hipStreamSynchronize(stream));
        prior_ready = false;
        prior_K = 0;
        prior_noise_valid = false;
        inj.erase(BBMPC_NOISE_POLICY);
        return;
    }
    check_dense_stack("policy prior: ", "n_layers must be >= 0", n_layers, dims, acts, w, b, is_normalized, stats, 4, [] {}, [&] {
        REQUIRE(dims[0] == S, BBMPC_E_INVALID,
                "policy prior: dims[0] = " + std::to_string(dims[0]) + " but the network reads the state, dim_s = " + std::to_string(S));
        REQUIRE(dims[n_layers] == U, BBMPC_E_INVALID,
                "policy prior: dims[n_layers] = " + std::to_string(dims[n_layers]) + " but the network returns an action, dim_u = " + std::to_string(U));
    });
    REQUIRE(std::isfinite(noise_std) && noise_std >= 0.0f, BBMPC_E_INVALID, "policy prior: noise_std must be finite and >= 0");
    REQUIRE(count >= 1, BBMPC_E_INVALID, "policy prior: count must be >= 1");
    for (int l = 1; l < n_layers; ++l) REQUIRE(dims[l] <= POLICY_MAX_HIDDEN, BBMPC_E_UNSUPPORTED, "hidden width > 512 not supported");
    REQUIRE(cfg.optimizer == BBMPC_OPT_CEM, BBMPC_E_UNSUPPORTED,
            "a policy prior with an optimizer other than CEM: only CEM's candidates are replaced between the draw and the rollout");
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_UNSUPPORTED,
            "a policy prior rolls the policy through a learned model: the handle needs BBMPC_DYN_MLP, not analytic or user dynamics");
    REQUIRE(!user_callbacks(), BBMPC_E_UNSUPPORTED, "a policy prior beside a callback plug-in: the step-wise rollout draws for itself");
    REQUIRE(!has_xform(), BBMPC_E_UNSUPPORTED,
            "a policy prior beside an inverse target transform: the policy rollout's model step is next = dev + state");
    REQUIRE(!pop_sharded() && cfg.population_global <= N && auto_split <= 1, BBMPC_E_UNSUPPORTED,
            "a policy prior with a sharded population: the sharded control steps draw inside their rollout kernels");
    REQUIRE(ens_E == 0 && lv_heads == 0, BBMPC_E_UNSUPPORTED,
            "a policy prior beside a model ensemble or log-variance heads: the policy rollout is the noise-free step of one model");
    REQUIRE((long)count + carry_stride() < (long)N, BBMPC_E_INVALID,
            "policy prior: count + max(keep_elites, shift_elites) = " + std::to_string((long)count + carry_stride()) +
                " must be below population_size = " + std::to_string(N));
    REQUIRE((long)A * count * HU < (1L << 31), BBMPC_E_UNSUPPORTED, "policy prior: more than 2^31 noise elements per iteration");
    MlpDesc d;
    const int pnw = dense_stack_shape(d, n_layers, dims);
    if (mlp_ready)
        REQUIRE((size_t)policy_prior_lds_layout(mlp, d, U, S, std::max(pnw, mlp_nw)).total * sizeof(float) <= 159 * 1024, BBMPC_E_UNSUPPORTED,
                "policy prior: the activation / partial-sum buffers of the two networks do not fit one CU's LDS");
    REQUIRE((size_t)policy_rows_lds_layout(d, U, S, pnw).total * sizeof(float) <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "policy prior: the activation / partial-sum buffers of this network do not fit one CU's LDS");
    std::vector<float> w4[MLP_MAX_LAYERS], bp[MLP_MAX_LAYERS], st;
    for (int l = 0; l < n_layers; ++l) {
        d.act[l] = acts[l];
        std::vector<float> wp;
        mlp_pack_layer(d, l, w[l], b[l], wp, w4[l], bp[l]);
    }
    if (is_normalized) {
        const int lens[4] = {S, S, U, U};
        for (int i = 0; i < 4; ++i) st.insert(st.end(), stats[i], stats[i] + lens[i]);
    }
    invalidate_step_graph();
    HIP_CHECK(hipStreamSynchronize(stream));
    prior_ready = false;
    if (count != prior_K) inj.erase(BBMPC_NOISE_POLICY);             // (its layout depends on K)
    for (int l = 0; l < n_layers; ++l) {
        upload(d_pr_wp4[l], w4[l]);
        upload(d_pr_bp[l], bp[l]);
        d.bpack[l] = d_pr_bp[l].p;
    }
    d.normalized = is_normalized ? 1 : 0;
    if (is_normalized) {
        upload(d_pr_stats, st);
        d.mean_s = d_pr_stats.p;
        d.std_s = d_pr_stats.p + S;
        d.mean_t = d_pr_stats.p + 2 * S;
        d.std_t = d_pr_stats.p + 2 * S + U;
    }
    const size_t ne = (size_t)A * count * HU;
    if (d_pr_noise.n < ne) d_pr_noise.alloc(ne);
    prior_mlp = d;
    prior_nw = pnw;
    prior_K = count;
    prior_sigma = noise_std;
    prior_noise_valid = false;
    prior_ready = true;
}

// xi [A][K][H][U] of (control step, iteration): the injected tensor, or the handle's own draws, generated once per
// (step, iteration)
const float* Engine::policy_noise(uint32_t step, uint32_t iter) {
    const size_t ne = (size_t)A * prior_K * HU;
    if (const float* in = injected(BBMPC_NOISE_POLICY)) return in + ne * std::min<size_t>(iter, (size_t)std::max(iters, 1) - 1);
    if (prior_noise_valid && prior_noise_step == step && prior_noise_iter == iter) return d_pr_noise.p;
    RngKey kk = key(step);
    kk.step_src = nullptr;
    const int blocks = A * prior_K * (int)kk.q_per_agent;
    hipLaunchKernelGGL(k_gen_policy_noise, dim3((blocks + 255) / 256), dim3(256), 0, stream, kk, iter, A, prior_K, HU, cfg.agent_offset,
                       d_pr_noise.p);
    HIP_CHECK(hipGetLastError());
    prior_noise_valid = true; prior_noise_step = step; prior_noise_iter = iter;
    return d_pr_noise.p;
}

void Engine::dump_policy_noise(int control_step, int iteration, float* out, int64_t count) {
    REQUIRE(prior_on(), BBMPC_E_STATE, "dump_noise: policy noise needs bbmpc_set_policy_prior_mlp first");
    const int64_t total = (int64_t)A * prior_K * HU;
    REQUIRE(count == total, BBMPC_E_INVALID, "dump_noise: policy noise is [A, K, H, U]");
    RngKey kk = key((uint32_t)control_step);
    kk.step_src = nullptr;
    const int blocks = A * prior_K * (int)kk.q_per_agent;
    stage_read_back(*this, out, (size_t)total, [&](float* d) {
        hipLaunchKernelGGL(k_gen_policy_noise, dim3((blocks + 255) / 256), dim3(256), 0, stream, kk, (uint32_t)iteration, A, prior_K, HU,
                           cfg.agent_offset, d);
    });
}

// The K policy rollouts of every agent from d_state [A][S]: into columns col0 .. col0 + K - 1 of `samples` [A][HU][nst]
// (the control step), into d_actions_out [K,A,H,U] / d_states_out [K,A,H,S] (bbmpc_predict_policy_rollouts), or both.
// One kernel, one instantiation per activation set, whoever calls.
void Engine::policy_prior_rollouts(const float* d_state, const float* d_noise, float* samples, int nst, int col0, float* d_actions_out,
                                   float* d_states_out) {
    REQUIRE(prior_ready, BBMPC_E_STATE, "policy prior: call bbmpc_set_policy_prior_mlp before computing");
    REQUIRE(mlp_ready, BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    const int K = prior_K;
    if (samples) REQUIRE(col0 >= 0 && col0 + K <= nst, BBMPC_E_INVALID, "internal: policy prior columns");
    PolicyPriorArgs q;
    memset(&q, 0, sizeof(q));
    q.m = mlp;
    q.pm = prior_mlp;
    for (int l = 0; l < mlp.n_layers; ++l) q.wp4[l] = d_wpack4[l].p;
    for (int l = 0; l < prior_mlp.n_layers; ++l) q.pwp4[l] = d_pr_wp4[l].p;
    q.nw = std::max(mlp_nw, prior_nw);
    q.K = K; q.A = A; q.H = H; q.S = S; q.U = U;
    q.Nst = nst; q.col0 = col0;
    q.sigma = prior_sigma;
    q.state = d_state;
    q.noise = d_noise;
    q.lo = d_lo.p; q.hi = d_hi.p;
    q.samples = samples;
    q.actions_out = d_actions_out;
    q.states_out = d_states_out;
    if (prior_sigma != 0.0f) REQUIRE(d_noise, BBMPC_E_INVALID, "internal: policy prior noise");
    const size_t lds = (size_t)policy_prior_lds_layout(mlp, prior_mlp, U, S, q.nw).total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED,
            "policy prior: the activation / partial-sum buffers of the two networks do not fit one CU's LDS");
    const bool ext = mlp_has_ext_act(mlp) || mlp_has_ext_act(prior_mlp);
    launch_args(ext ? k_policy_prior_rollout<true> : k_policy_prior_rollout<false>, dim3((K + MLP_TP - 1) / MLP_TP, A), dim3(q.nw * 64), lds, stream, q);
}

// pi on B rows of states [B][S] -> actions [B][U]: no noise, no clip
void Engine::policy_prior_rows(const float* d_states, int batch, float* d_actions) {
    REQUIRE(prior_ready, BBMPC_E_STATE, "policy prior: call bbmpc_set_policy_prior_mlp before computing");
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    PolicyRowsArgs q;
    memset(&q, 0, sizeof(q));
    q.pm = prior_mlp;
    for (int l = 0; l < prior_mlp.n_layers; ++l) q.pwp4[l] = d_pr_wp4[l].p;
    q.nw = prior_nw;
    q.B = batch; q.S = S; q.U = U;
    q.states = d_states;
    q.actions = d_actions;
    const size_t lds = (size_t)policy_rows_lds_layout(prior_mlp, U, S, prior_nw).total * sizeof(float);
    launch_args(mlp_has_ext_act(prior_mlp) ? k_policy_prior_rows<true> : k_policy_prior_rows<false>, dim3((batch + MLP_TP - 1) / MLP_TP),
                dim3(prior_nw * 64), lds, stream, q);
}


// ------------------------------------------------------------------------------------------------
// plan gradients (bbmpc_plan_gradient; kernels_plan_grad.hpp)
// ------------------------------------------------------------------------------------------------
// W and W^T of every layer of network `which` (0 dynamics, 1 reward, 2 value), both through mlp_pack_layer, features in
// index order, into the feature's own buffers; the reversed network's biases are one shared block of zeros.
void Engine::plan_gradient_pack(int which) {
    const PgHostNet& hn = pg_host[which];
    PgNet n;
    memset(&n, 0, sizeof(n));
    const int L = hn.L;
    n.f.n_layers = n.r.n_layers = L;
    for (int l = 0; l <= L; ++l) {
        n.f.dims[l] = hn.dims[l];
        n.f.tiles[l] = (hn.dims[l] + 15) / 16;
        n.r.dims[L - l] = n.f.dims[l];
        n.r.tiles[L - l] = n.f.tiles[l];
        if (l >= 1 && l < L) n.hid += n.f.tiles[l];
    }
    if (d_pg_zero.n == 0) {
        d_pg_zero.alloc(2 * 16 * MLP_TMAX * 256);
        HIP_CHECK(hipMemset(d_pg_zero.p, 0, d_pg_zero.n * sizeof(float)));
    }
    for (int l = 0; l < L; ++l) {
        n.act[l] = hn.acts[l];
        std::vector<float> wp, w4, bp;
        mlp_pack_layer(n.f, l, hn.w[l].data(), hn.b[l].data(), wp, w4, bp);
        upload(d_pg_wf[which][l], w4);
        upload(d_pg_bf[which][l], bp);
        n.wf[l] = d_pg_wf[which][l].p;
        n.f.bpack[l] = d_pg_bf[which][l].p;
        const int j = L - 1 - l, K = hn.dims[l], M = hn.dims[l + 1];       // reversed layer j: [M][K]
        std::vector<float> wt((size_t)M * K), zb((size_t)K, 0.0f);
        for (int k = 0; k < K; ++k)
            for (int o = 0; o < M; ++o) wt[(size_t)o * K + k] = hn.w[l][(size_t)k * M + o];
        mlp_pack_layer(n.r, j, wt.data(), zb.data(), wp, w4, bp);
        upload(d_pg_wr[which][j], w4);
        n.wr[j] = d_pg_wr[which][j].p;
        n.r.bpack[j] = d_pg_zero.p;
    }
    pg_net[which] = n;
    pg_stale[which] = false;
}

// Every refusal of a gradient call, the launch shape and the sizes -- before anything is allocated or packed.
void Engine::plan_gradient_check(int batch, int horizon, PlanGradArgs& q, size_t& lds, size_t& ws_floats) {
    plan_gradient_eligible();
    plan_gradient_sizes(batch, horizon, q, lds, ws_floats);
}

void Engine::plan_gradient_eligible() const {
    REQUIRE(cfg.dynamics == BBMPC_DYN_MLP, BBMPC_E_UNSUPPORTED,
            "plan gradient: the return is differentiated through a learned model: the handle needs BBMPC_DYN_MLP, not analytic or user dynamics");
    REQUIRE(cfg.reward == BBMPC_REW_MLP, BBMPC_E_UNSUPPORTED,
            "plan gradient: the reward must be a learned reward network (BBMPC_REW_MLP), not a built-in or HIP-source reward");
    REQUIRE(ens_E == 0 && lv_heads == 0, BBMPC_E_UNSUPPORTED,
            "plan gradient beside a model ensemble or log-variance heads: the gradient is that of one noise-free model");
    REQUIRE(!has_xform(), BBMPC_E_UNSUPPORTED, "plan gradient beside an inverse target transform: the differentiated step is next = dev + state");
    REQUIRE(!user_callbacks(), BBMPC_E_UNSUPPORTED, "plan gradient beside a callback plug-in: a callback has no derivative");
    REQUIRE(!shaping_on(), BBMPC_E_UNSUPPORTED,
            "plan gradient beside return shaping (bbmpc_set_return_shaping): the differentiated return is the undiscounted sum over the "
            "full horizon, not the shaped one; switch shaping off first (discount = 1, no bounds)");
}

void Engine::plan_gradient_sizes(int batch, int horizon, PlanGradArgs& q, size_t& lds, size_t& ws_floats) {
    REQUIRE(mlp_ready, BBMPC_E_STATE, "plan gradient: learned dynamics not set: call bbmpc_set_mlp before computing");
    REQUIRE(rew_mlp_ready, BBMPC_E_STATE, "plan gradient: learned reward not set: call bbmpc_set_reward_mlp before computing");
    REQUIRE(batch >= 1, BBMPC_E_INVALID, "batch must be >= 1");
    REQUIRE(horizon >= 1 && horizon <= 4096, BBMPC_E_INVALID, "horizon must be in [1, 4096]");
    memset(&q, 0, sizeof(q));
    // the shapes alone decide the sizes: taken from the host copies, so that nothing has to be packed to refuse
    PgNet shape[3];
    memset(shape, 0, sizeof(shape));
    int hidden_tiles = 1;
    for (int i = 0; i < 3; ++i) {
        if (i == 2 && !val_mlp_ready) continue;
        const PgHostNet& hn = pg_host[i];
        shape[i].f.n_layers = hn.L;
        for (int l = 0; l <= hn.L; ++l) {
            shape[i].f.dims[l] = hn.dims[l];
            shape[i].f.tiles[l] = (hn.dims[l] + 15) / 16;
            if (l >= 1 && l < hn.L) {
                shape[i].hid += shape[i].f.tiles[l];
                hidden_tiles = std::max(hidden_tiles, shape[i].f.tiles[l]);
            }
        }
    }
    q.has_val = val_mlp_ready ? 1 : 0;
    q.nw = std::min(16, hidden_tiles);
    q.B = batch; q.Hq = horizon; q.S = S; q.U = U;
    q.r_D = rew_mlp.D;
    lds = (size_t)plan_grad_lds_layout(shape[0], shape[1], shape[2], q.has_val, S, U, rew_mlp.D).total * sizeof(float);
    REQUIRE(lds <= 159 * 1024, BBMPC_E_UNSUPPORTED, "plan gradient: the activation buffers of the three networks do not fit one CU's LDS");
    q.step_stride = plan_grad_step_stride(shape[0].hid, shape[1].hid, S);
    const long tiles = (batch + MLP_TP - 1) / MLP_TP;
    const long tile_stride = (long)horizon * q.step_stride + (q.has_val ? shape[2].hid * 256 : 0);
    REQUIRE(tiles * tile_stride < (1L << 31), BBMPC_E_UNSUPPORTED,
            "plan gradient: the workspace of this batch and horizon has 2^31 elements or more (split the batch)");
    q.tile_stride = (int)tile_stride;
    ws_floats = (size_t)(tiles * tile_stride);
}

void Engine::plan_gradient_dev(const float* d_states, const float* d_seq, int batch, int horizon, float* d_returns, float* d_grad) {
    PlanGradArgs q;
    size_t lds = 0, wsn = 0;
    plan_gradient_check(batch, horizon, q, lds, wsn);
    plan_gradient_prepare(wsn);
    plan_gradient_launch(q, lds, d_states, d_seq, d_returns, d_grad);
}

// W / W^T of a network installed since the last call, and the workspace: everything of a gradient call that may wait for
// the stream or allocate
void Engine::plan_gradient_prepare(size_t wsn) {
    for (int i = 0; i < 3; ++i)
        if (pg_stale[i] && (i < 2 || val_mlp_ready)) {
            HIP_CHECK(hipStreamSynchronize(stream));               // (a call in flight may still read the old operands)
            plan_gradient_pack(i);
        }
    if (d_pg_ws.n < wsn) {
        HIP_CHECK(hipStreamSynchronize(stream));
        d_pg_ws.alloc(wsn);
    }
}

// One launch of k_plan_grad on checked arguments (q from plan_gradient_check, after plan_gradient_prepare)
void Engine::plan_gradient_launch(PlanGradArgs q, size_t lds, const float* d_states, const float* d_seq, float* d_returns, float* d_grad) {
    const int batch = q.B;
    q.dyn = pg_net[0];
    q.dyn.f.normalized = mlp.normalized;
    q.dyn.f.mean_s = mlp.mean_s; q.dyn.f.std_s = mlp.std_s;
    q.dyn.f.mean_a = mlp.mean_a; q.dyn.f.std_a = mlp.std_a;
    q.dyn.f.mean_t = mlp.mean_t; q.dyn.f.std_t = mlp.std_t;
    q.rew = pg_net[1];
    q.r_norm = rew_mlp.normalized; q.r_mask = rew_mlp.mask; q.r_off_a = rew_mlp.off_a; q.r_off_n = rew_mlp.off_n;
    q.r_mean = rew_mlp.mean_in; q.r_std = rew_mlp.std_in;
    q.r_mean_out = rew_mlp.mean_r; q.r_std_out = rew_mlp.std_r;
    if (q.has_val) {
        q.val = pg_net[2];
        q.w = val_weight;
        q.v_norm = val_mlp.normalized;
        q.v_mean = val_mlp.mean_in; q.v_std = val_mlp.std_in;
        q.v_mean_out = val_mlp.mean_r; q.v_std_out = val_mlp.std_r;
    }
    q.states = d_states;
    q.seq = d_seq;
    q.returns_out = d_returns;
    q.grad_out = d_grad;
    q.ws = d_pg_ws.p;
    launch_args(k_plan_grad, dim3((batch + MLP_TP - 1) / MLP_TP), dim3(q.nw * 64), lds, stream, q);
}

// ------------------------------------------------------------------------------------------------
// plan refinement on the device (bbmpc_refine_plans, bbmpc_set_grad_refine; kernels_plan_refine.hpp)
// ------------------------------------------------------------------------------------------------
void Engine::refine_plans_check(int batch, int horizon, int steps, float lr, int method, int keep_best, PlanGradArgs& q, size_t& lds,
                                size_t& wsn) {
    plan_gradient_check(batch, horizon, q, lds, wsn);
    REQUIRE(steps >= 0 && steps <= REFINE_MAX_STEPS, BBMPC_E_INVALID, "refine plans: steps must be in [0, 64]");
    REQUIRE(std::isfinite(lr) && lr > 0.0f, BBMPC_E_INVALID, "refine plans: lr must be finite and positive");
    REQUIRE(method == REFINE_ADAM || method == REFINE_SGD, BBMPC_E_INVALID, "refine plans: method must be 0 (adam) or 1 (sgd)");
    REQUIRE(keep_best == 0 || keep_best == 1, BBMPC_E_INVALID, "refine plans: keep_best must be 0 or 1");
}

void Engine::refine_plans_dev(const float* d_states, float* d_seq, int batch, int horizon, int steps, float lr, int method, int keep_best,
                              float* d_returns_out) {
    PlanGradArgs q;
    size_t lds = 0, wsn = 0;
    refine_plans_check(batch, horizon, steps, lr, method, keep_best, q, lds, wsn);
    refine_plans_run(q, lds, wsn, d_states, d_seq, steps, lr, method, keep_best, d_returns_out);
}

// The loop on checked arguments (q, lds, wsn from refine_plans_check: no check is repeated per step).  d_seq [B, Hq, U] is
// refined in place.  keep_best: steps + 1 gradient calls, the best plan per row by model return (the input included) into
// d_seq, its return into d_returns_out.  Otherwise steps gradient calls, the last iterate stays in d_seq, and d_returns_out
// (when not null) costs one more call that scores it.
void Engine::refine_plans_run(const PlanGradArgs& q, size_t lds, size_t wsn, const float* d_states, float* d_seq, int steps, float lr, int method,
                              int keep_best, float* d_returns_out) {
    const int batch = q.B, horizon = q.Hq;
    // everything that allocates or packs, before the first launch: from here on no synchronisation and no host visit
    plan_gradient_prepare(wsn);
    const size_t n = (size_t)batch * horizon * U, np4 = (n + 3) & ~(size_t)3, nb = ((size_t)batch + 3) & ~(size_t)3;
    if (d_rf.n < 4 * np4 + 2 * nb) {
        HIP_CHECK(hipStreamSynchronize(stream));
        d_rf.alloc(4 * np4 + 2 * nb);
    }
    float* g = d_rf.p;
    float* m = g + np4;
    float* v = m + np4;
    float* best = v + np4;
    float* ret = best + np4;
    float* best_ret = ret + nb;
    if (method == REFINE_ADAM && steps > 0) HIP_CHECK(hipMemsetAsync(m, 0, 2 * np4 * sizeof(float), stream));
    RefineStepArgs a;
    a.x = d_seq; a.g = g; a.m = m; a.v = v;
    a.lo = d_lo.p; a.hi = d_hi.p;
    a.n = (long)n; a.U = U; a.method = method; a.lr = lr;
    const bool v4 = n % 4 == 0 && ((uintptr_t)d_seq & 15) == 0;      // (the handle's own buffers are 16-byte aligned)
    const int row = horizon * U;
    for (int k = 0; k <= steps; ++k) {
        if (k == steps && !keep_best && !d_returns_out) break;
        plan_gradient_launch(q, lds, d_states, d_seq, (k == steps && !keep_best) ? d_returns_out : ret, g);
        if (keep_best) {
            hipLaunchKernelGGL(k_refine_keep_best, dim3(batch), dim3(64), 0, stream, (const float*)d_seq, (const float*)ret, best, best_ret, row,
                               k == 0 ? 1 : 0);
            HIP_CHECK(hipGetLastError());
        }
        if (k == steps) break;
        refine_bias_correction(k + 1, a.c1, a.c2);
        if (v4) hipLaunchKernelGGL(k_refine_step<true>, dim3((unsigned)((n / 4 + REFINE_THREADS - 1) / REFINE_THREADS)), dim3(REFINE_THREADS), 0, stream, a);
        else hipLaunchKernelGGL(k_refine_step<false>, dim3((unsigned)((n + REFINE_THREADS - 1) / REFINE_THREADS)), dim3(REFINE_THREADS), 0, stream, a);
        HIP_CHECK(hipGetLastError());
    }
    if (keep_best) {
        HIP_CHECK(hipMemcpyAsync(d_seq, best, n * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (d_returns_out) HIP_CHECK(hipMemcpyAsync(d_returns_out, best_ret, (size_t)batch * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
}

// bbmpc_set_grad_refine.  Everything that can be refused is refused before the handle changes.
void Engine::set_grad_refine(int steps, float lr, int method, int candidates) {
    REQUIRE(cfg.optimizer == BBMPC_OPT_CEM, BBMPC_E_UNSUPPORTED,
            "gradient refinement with an optimizer other than CEM: only CEM's candidates are refined between the draw and the rollout");
    if (steps == 0) {
        if (grad_on()) invalidate_step_graph();
        gr_steps = 0;
        return;
    }
    REQUIRE(steps >= 1 && steps <= REFINE_MAX_STEPS, BBMPC_E_INVALID, "gradient refinement: steps must be in [0, 64]");
    REQUIRE(std::isfinite(lr) && lr > 0.0f, BBMPC_E_INVALID, "gradient refinement: lr must be finite and positive");
    REQUIRE(method == REFINE_ADAM || method == REFINE_SGD, BBMPC_E_INVALID, "gradient refinement: method must be 0 (adam) or 1 (sgd)");
    REQUIRE(candidates >= 0 && candidates <= N, BBMPC_E_INVALID,
            "gradient refinement: candidates must be in [0, population_size = " + std::to_string(N) + "] (0: all)");
    REQUIRE(!particles_on(), BBMPC_E_UNSUPPORTED,
            "gradient refinement with particles (bbmpc_set_particles): the gradient is that of one noise-free rollout");
    REQUIRE(!pop_sharded() && cfg.population_global <= N && auto_split <= 1, BBMPC_E_UNSUPPORTED,
            "gradient refinement with a sharded population: the sharded control steps draw inside their rollout kernels");
    plan_gradient_eligible();
    invalidate_step_graph();
    gr_steps = steps; gr_lr = lr; gr_method = method; gr_M = candidates;
}

// Columns [N - M, N) of every agent's candidates: out of the sample buffer into rows, gr_steps gradient steps from the
// agent's state (refine_plans_dev, keep_best = 0, no returns), back over the same columns.
void Engine::grad_refine_candidates(RolloutArgs& ra) {
    REQUIRE(ra.n_pop == N && ra.HU == HU && ra.H == H && ra.Nst == Nst && ra.samples, BBMPC_E_INVALID, "internal: gradient refinement shape");
    const int M = gr_M > 0 ? gr_M : N;
    const int B = A * M;
    PlanGradArgs q;
    size_t lds = 0, wsn = 0;
    refine_plans_check(B, H, gr_steps, gr_lr, gr_method, 0, q, lds, wsn);    // (networks not installed: BBMPC_E_STATE, before anything is allocated)
    if (d_gr_rows.n < (size_t)B * HU || d_gr_states.n < (size_t)B * S) {
        HIP_CHECK(hipStreamSynchronize(stream));
        d_gr_rows.alloc((size_t)B * HU);
        d_gr_states.alloc((size_t)B * S);
    }
    hipLaunchKernelGGL(k_refine_gather, dim3((HU * M + S * M + REFINE_THREADS - 1) / REFINE_THREADS, A), dim3(REFINE_THREADS), 0, stream,
                       (const float*)ra.samples, ra.state, d_gr_rows.p, d_gr_states.p, HU, S, Nst, N, M);
    HIP_CHECK(hipGetLastError());
    refine_plans_run(q, lds, wsn, d_gr_states.p, d_gr_rows.p, gr_steps, gr_lr, gr_method, 0, nullptr);
    hipLaunchKernelGGL(k_refine_scatter, dim3((HU * M + REFINE_THREADS - 1) / REFINE_THREADS, A), dim3(REFINE_THREADS), 0, stream,
                       (const float*)d_gr_rows.p, ra.samples, HU, Nst, N, M);
    HIP_CHECK(hipGetLastError());
}

}  // namespace bbmpc

extern "C" int bbmpc_refine_plans_dev(bbmpc_handle h, const float* d_states, float* d_seq, int32_t batch, int32_t horizon, int32_t steps,
                                      float lr, int32_t method, int32_t keep_best, float* d_returns_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_seq);
    h->e->refine_plans_dev(d_states, d_seq, batch, horizon, steps, lr, method, keep_best, d_returns_out);
    API_END
}

extern "C" int bbmpc_refine_plans(bbmpc_handle h, const float* states, float* seq, int32_t batch, int32_t horizon, int32_t steps, float lr,
                                  int32_t method, int32_t keep_best, float* returns_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(seq);
    bbmpc::Engine& e = *h->e;
    bbmpc::PlanGradArgs q;
    size_t lds = 0, wsn = 0;
    e.refine_plans_check(batch, horizon, steps, lr, method, keep_best, q, lds, wsn);     // every refusal before the staging buffer is touched
    HostStage st(e);
    const int s = st.in(states, (size_t)batch * e.S), p = st.inout(seq, (size_t)batch * horizon * e.U, bbmpc::StageLayout::kVec4);
    const int r = st.out(returns_out, (size_t)batch);                       // (the plans: k_refine_step's float4 form wants 16 bytes)
    st.upload();
    e.refine_plans_run(q, lds, wsn, st[s], st[p], steps, lr, method, keep_best, st[r]);
    st.finish();
    API_END
}

extern "C" int bbmpc_set_grad_refine(bbmpc_handle h, int32_t steps, float lr, int32_t method, int32_t candidates) {
    API_BEGIN
    CHECK_HANDLE(h);                     // (settles the handle: a resident control-step kernel is stopped first)
    h->e->set_grad_refine(steps, lr, method, candidates);
    API_END
}

extern "C" int bbmpc_get_grad_refine(bbmpc_handle h, int32_t* steps, float* lr, int32_t* method, int32_t* candidates) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(steps);
    CHECK_PTR(lr);
    CHECK_PTR(method);
    CHECK_PTR(candidates);
    const bbmpc::Engine& e = *h->e;
    *steps = e.gr_steps;
    *lr = e.grad_on() ? e.gr_lr : 0.0f;
    *method = e.grad_on() ? e.gr_method : 0;
    *candidates = e.grad_on() ? e.gr_M : 0;
    API_END
}

extern "C" int bbmpc_set_policy_prior_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* acts, const float* const* w,
                                          const float* const* b, int32_t is_normalized, const float* const* stats, int32_t count,
                                          float noise_std) {
    API_BEGIN
    CHECK_HANDLE(h);                     // (settles the handle: a resident control-step kernel is stopped first)
    h->e->set_policy_prior_mlp(n_layers, dims, acts, w, b, is_normalized, stats, count, noise_std);
    API_END
}

extern "C" int bbmpc_get_policy_prior(bbmpc_handle h, int32_t* count, float* noise_std) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(count);
    CHECK_PTR(noise_std);
    *count = h->e->prior_on() ? h->e->prior_K : 0;
    *noise_std = h->e->prior_on() ? h->e->prior_sigma : 0.0f;
    if (!h->e->prior_on()) throw bbmpc::HipError(BBMPC_E_STATE, "policy prior: no network installed");
    API_END
}

extern "C" int bbmpc_evaluate_policy_prior_dev(bbmpc_handle h, const float* d_states, int32_t batch, float* d_actions) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_actions);
    h->e->policy_prior_rows(d_states, batch, d_actions);
    API_END
}

extern "C" int bbmpc_evaluate_policy_prior(bbmpc_handle h, const float* states, int32_t batch, float* actions) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(actions);
    bbmpc::Engine& e = *h->e;
    if (batch < 1) throw bbmpc::HipError(BBMPC_E_INVALID, "batch must be >= 1");
    if (!e.prior_on()) throw bbmpc::HipError(BBMPC_E_STATE, "policy prior: call bbmpc_set_policy_prior_mlp before computing");
    HostStage st(e);
    const int s = st.in(states, (size_t)batch * e.S), a = st.out(actions, (size_t)batch * e.U);
    st.upload();
    e.policy_prior_rows(st[s], batch, st[a]);
    st.finish();
    API_END
}

extern "C" int bbmpc_predict_policy_rollouts_dev(bbmpc_handle h, const float* d_states, const float* d_noise, float* d_actions_out,
                                                 float* d_states_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    bbmpc::Engine& e = *h->e;
    if (!d_actions_out && !d_states_out) throw bbmpc::HipError(BBMPC_E_INVALID, "policy rollouts: actions_out and states_out are both NULL");
    if (!e.prior_on()) throw bbmpc::HipError(BBMPC_E_STATE, "policy prior: call bbmpc_set_policy_prior_mlp before computing");
    if (!d_noise && e.prior_sigma != 0.0f) d_noise = e.policy_noise(e.step_counter, 0);
    e.policy_prior_rollouts(d_states, d_noise, nullptr, 0, 0, d_actions_out, d_states_out);
    API_END
}

extern "C" int bbmpc_predict_policy_rollouts(bbmpc_handle h, const float* states, const float* noise, float* actions_out, float* states_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    bbmpc::Engine& e = *h->e;
    if (!actions_out && !states_out) throw bbmpc::HipError(BBMPC_E_INVALID, "policy rollouts: actions_out and states_out are both NULL");
    if (!e.prior_on()) throw bbmpc::HipError(BBMPC_E_STATE, "policy prior: call bbmpc_set_policy_prior_mlp before computing");
    if (!e.mlp_ready) throw bbmpc::HipError(BBMPC_E_STATE, "learned dynamics: call bbmpc_set_mlp before computing");
    HostStage st(e);
    const int s = st.in(states, (size_t)e.A * e.S), n = st.in(noise, (size_t)e.A * e.prior_K * e.HU);
    const int a = st.out(actions_out, (size_t)e.prior_K * e.A * e.HU), so = st.out(states_out, (size_t)e.prior_K * e.A * e.H * e.S);
    st.upload();
    const float* use = noise ? st[n] : (e.prior_sigma != 0.0f ? e.policy_noise(e.step_counter, 0) : nullptr);
    e.policy_prior_rollouts(st[s], use, nullptr, 0, 0, st[a], st[so]);
    st.finish();
    API_END
}

extern "C" int bbmpc_set_reward_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* acts, const float* const* w,
                                    const float* const* b, int32_t input_mask, int32_t is_normalized, const float* const* stats) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_reward_mlp(n_layers, dims, acts, w, b, input_mask, is_normalized, stats);
    API_END
}

extern "C" int bbmpc_set_terminal_value_mlp(bbmpc_handle h, int32_t n_layers, const int32_t* dims, const int32_t* acts, const float* const* w,
                                            const float* const* b, int32_t is_normalized, const float* const* stats, float terminal_weight) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_terminal_value_mlp(n_layers, dims, acts, w, b, is_normalized, stats, terminal_weight);
    API_END
}

extern "C" int bbmpc_evaluate_terminal_value_dev(bbmpc_handle h, const float* d_states, int32_t batch, float* d_values) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_values);
    h->e->terminal_value_rows(d_states, batch, d_values);
    API_END
}

extern "C" int bbmpc_evaluate_terminal_value(bbmpc_handle h, const float* states, int32_t batch, float* values) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(values);
    bbmpc::Engine& e = *h->e;
    if (batch < 1) throw bbmpc::HipError(BBMPC_E_INVALID, "batch must be >= 1");
    if (!e.val_mlp_ready) throw bbmpc::HipError(BBMPC_E_STATE, "terminal value: call bbmpc_set_terminal_value_mlp before computing");
    HostStage st(e);
    const int s = st.in(states, (size_t)batch * e.S), v = st.out(values, (size_t)batch);
    st.upload();
    e.terminal_value_rows(st[s], batch, st[v]);
    st.finish();
    API_END
}

extern "C" int bbmpc_set_return_shaping(bbmpc_handle h, float discount, const float* state_lo, const float* state_hi, float terminal_reward) {
    API_BEGIN
    CHECK_HANDLE(h);
    h->e->set_return_shaping(discount, state_lo, state_hi, terminal_reward);
    API_END
}

extern "C" int bbmpc_get_termination_steps(bbmpc_handle h, int32_t* out, int32_t n) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(out);
    h->e->termination_steps(out, n);
    API_END
}

extern "C" int bbmpc_plan_gradient_dev(bbmpc_handle h, const float* d_states, const float* d_seq, int32_t batch, int32_t horizon,
                                       float* d_returns_out, float* d_grad_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(d_states);
    CHECK_PTR(d_seq);
    CHECK_PTR(d_grad_out);
    h->e->plan_gradient_dev(d_states, d_seq, batch, horizon, d_returns_out, d_grad_out);
    API_END
}

extern "C" int bbmpc_plan_gradient(bbmpc_handle h, const float* states, const float* seq, int32_t batch, int32_t horizon, float* returns_out,
                                   float* grad_out) {
    API_BEGIN
    CHECK_HANDLE(h);
    CHECK_PTR(states);
    CHECK_PTR(seq);
    CHECK_PTR(grad_out);
    bbmpc::Engine& e = *h->e;
    {   // every refusal before the staging buffer is touched
        bbmpc::PlanGradArgs q;
        size_t lds = 0, wsn = 0;
        e.plan_gradient_check(batch, horizon, q, lds, wsn);
    }
    const size_t nq = (size_t)batch * horizon * e.U;
    HostStage st(e);
    const int s = st.in(states, (size_t)batch * e.S), p = st.in(seq, nq);
    const int g = st.out(grad_out, nq), r = st.out(returns_out, (size_t)batch);
    st.upload();
    e.plan_gradient_dev(st[s], st[p], batch, horizon, st[r], st[g]);
    st.finish();
    API_END
}
