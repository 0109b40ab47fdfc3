// Training a Dense stack through the C ABI (bbmpc_trainer_*): the host side of kernels_train.hpp.
// A trainer is independent of the planning handle: its own device, stream and buffers, no bbmpc_config.  It holds E >= 1
// equally shaped members (bbmpc_trainer_create: one; bbmpc_trainer_create_ensemble: up to 8) that step side by side, the
// member index being the kernels' second grid dimension.  bbmpc_trainer_create_gaussian: members with a log-variance head,
// fitted on the Gaussian NLL by the kernels' NLL instantiations.
#define BBMPC_TU_TRAIN
#include <cmath>
#include <limits>

#include "abi_util.hpp"
#include "kernels_train.hpp"

namespace bbmpc {

// Everything bbmpc_trainer_create refuses, checked before a device is touched.  Fills the layout.
static void train_describe(TrainNet& n, int32_t n_layers, const int32_t* dims, const int32_t* acts) {
    REQUIRE(n_layers >= 1, BBMPC_E_INVALID, "trainer: n_layers must be >= 1");
    REQUIRE(n_layers <= TR_MAX_LAYERS, BBMPC_E_UNSUPPORTED, "trainer: more than 8 layers");
    REQUIRE(dims && acts, BBMPC_E_INVALID, "trainer: null dims / activations");
    memset(&n, 0, sizeof(n));
    n.L = n_layers;
    for (int l = 0; l <= n_layers; ++l) {
        REQUIRE(dims[l] >= 1, BBMPC_E_INVALID, "trainer: a layer width < 1");
        n.dims[l] = dims[l];
    }
    for (int l = 0; l < n_layers; ++l) {
        REQUIRE(acts[l] >= ACT_NONE && acts[l] <= ACT_RELU6, BBMPC_E_INVALID, "trainer: unknown activation code");
        n.act[l] = acts[l];
    }
    for (int l = 0; l <= n_layers; ++l) REQUIRE(dims[l] <= TR_MAX_WIDTH, BBMPC_E_UNSUPPORTED, "trainer: a layer width > 512");
    int o = 0;
    for (int l = 0; l < n_layers; ++l) { n.woff[l] = o; o += n.dims[l] * n.dims[l + 1]; }
    for (int l = 0; l < n_layers; ++l) { n.boff[l] = o; o += n.dims[l + 1]; }
    n.n_params = o;
    train_lds_layout(n);
    REQUIRE((size_t)n.lds_floats * 4 <= (size_t)TR_LDS_LIMIT, BBMPC_E_UNSUPPORTED,
            "trainer: the network's resident layer tiles need " + std::to_string((size_t)n.lds_floats * 4) +
                " bytes of LDS, over the 159 KiB limit");
}

// train_describe for a network with a log-variance head (bbmpc_trainer_create_gaussian): W_v and b_v
// close theta, the head's z joins the carve, and the 159 KiB limit is checked on that carve -- before anything is allocated.
static void train_describe_head(TrainNet& n, TrainHead& h) {
    memset(&h, 0, sizeof(h));
    const int hidden = n.dims[n.L - 1], O = n.dims[n.L];
    h.woff = n.n_params;
    h.boff = h.woff + hidden * O;
    n.n_params = h.boff + O;
    train_lds_layout_head(n, h);
    REQUIRE((size_t)n.lds_floats * 4 <= (size_t)TR_LDS_LIMIT, BBMPC_E_UNSUPPORTED,
            "trainer: the network's resident layer tiles and the log-variance head need " + std::to_string((size_t)n.lds_floats * 4) +
                " bytes of LDS, over the 159 KiB limit");
}

// The bounds rule of bbmpc_set_mlp_logvar_head.
static void train_check_logvar_bounds(const float* lo, const float* hi, int O) {
    REQUIRE(lo && hi, BBMPC_E_INVALID, "trainer: null min_logvar / max_logvar");
    for (int o = 0; o < O; ++o)
        REQUIRE(std::isfinite(lo[o]) && std::isfinite(hi[o]) && std::fabs(lo[o]) <= 40.0f && std::fabs(hi[o]) <= 40.0f && lo[o] <= hi[o],
                BBMPC_E_INVALID, "trainer: min_logvar / max_logvar must be finite, within [-40, 40], with min_logvar <= max_logvar");
}

// The seed member e draws its permutations from when bbmpc_trainer_fit_ensemble is given none (member 0: the seed itself).
static inline uint64_t train_member_seed(uint64_t seed, int e) { return seed ^ (0x9E3779B97F4A7C15ull * (uint64_t)e); }

struct Trainer {
    int device = 0;
    int E = 1;                                   // members
    hipStream_t stream = nullptr;
    TrainNet net;                                // wf / wr / bp: member 0's; member e's lie e * net.pstride floats further
    bool gauss = false;                          // a log-variance head: the NLL instantiations of the kernels
    TrainHead head;                              // all zero without one
    DevBuf<float> lvb;                           // [2][O]: min_logvar, max_logvar
    int rule = TR_RULE_ADAM;
    double lr = 1e-3;
    DevBuf<float> theta, m, v;                   // [E][n_params]
    DevBuf<float> packs;                         // [E][pstride]: per member every layer's W pack, W^T pack, padded bias
    DevBuf<double> pows;                         // [E][2][2]
    long long steps = 0;                         // the members step together
    DevBuf<float> din, dout, vin, vout;          // the dataset, once for all members
    int n_train = 0, n_val = 0;
    bool has_data = false;
    std::vector<int32_t> member_rows;            // [E][n_train] training rows of each member; empty: identity
    DevBuf<float> part, lossp, loss_acc, val_loss, val_tiles, val_batch, grads, colsq, rms, rin, rout;
    DevBuf<int> perms, idx;
    // weight decay, early stopping, best-weights restore; they hold from fit to fit
    float wd[TR_MAX_LAYERS] = {0};               // lambda_l; all zero: off
    int wd_mode = TR_DECAY_L2;
    int patience = 0;
    float min_delta = 0.0f;
    bool restore_best = false;
    DevBuf<TrainMon> mon;                        // [E][2]
    DevBuf<float> best_theta;                    // [E][n_params]
    std::vector<TrainMon> mon_host;              // what a fit uploads to mon and reads back from it
    std::vector<int32_t> rep_epochs, rep_best_epoch;      // the last fit's report, [E]
    std::vector<float> rep_best_val;

    // weights / biases: [E * L] host arrays, member major.  hd (train_describe_head's, or null): the head, with head_w /
    // head_b [E] host arrays and the bounds lo / hi [O].
    Trainer(const TrainNet& n, int dev, int members, const float* const* weights, const float* const* biases, int rule_, double lr_,
            const TrainHead* hd = nullptr, const float* const* head_w = nullptr, const float* const* head_b = nullptr,
            const float* lo = nullptr, const float* hi = nullptr)
        : device(dev), E(members), net(n), gauss(hd != nullptr), rule(rule_), lr(lr_) {
        memset(&head, 0, sizeof(head));
        if (hd) head = *hd;
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        const int L = net.L;
        const size_t np = (size_t)net.n_params;
        // one slab of operand packs per member: [wf_0 wr_0 bp_0 .. wf_{L-1} wr_{L-1} bp_{L-1}] and then the head's [wf_v wr_v
        // bp_v], every piece a multiple of 16 floats
        size_t off_f[TR_MAX_LAYERS + 1], off_r[TR_MAX_LAYERS + 1], off_b[TR_MAX_LAYERS + 1], slab = 0;
        for (int l = 0; l < L + (gauss ? 1 : 0); ++l) {
            const int ll = l < L ? l : L - 1;    // the head has the last layer's shape
            const size_t pack = (size_t)net.tiles[ll] * net.tiles[ll + 1] * 256;
            off_f[l] = slab; slab += pack;
            off_r[l] = slab; slab += pack;
            off_b[l] = slab; slab += (size_t)net.tiles[ll + 1] * 16;
        }
        net.pstride = (int)slab;
        std::vector<float> h(np * E), s(slab * E, 0.0f);
        for (int e = 0; e < E; ++e)
            for (int l = 0; l < L; ++l) {
                const int in = net.dims[l], out = net.dims[l + 1], IT = net.tiles[l], OT = net.tiles[l + 1];
                const float* w = weights[(size_t)e * L + l];
                const float* b = biases[(size_t)e * L + l];
                memcpy(h.data() + e * np + net.woff[l], w, sizeof(float) * in * out);
                memcpy(h.data() + e * np + net.boff[l], b, sizeof(float) * out);
                float* f = s.data() + e * slab + off_f[l];
                float* r = s.data() + e * slab + off_r[l];
                for (int i = 0; i < in; ++i)
                    for (int o = 0; o < out; ++o) {
                        f[train_wf_index(IT, i, o)] = w[(size_t)i * out + o];
                        r[train_wr_index(OT, i, o)] = w[(size_t)i * out + o];
                    }
                memcpy(s.data() + e * slab + off_b[l], b, sizeof(float) * out);
            }
        for (int e = 0; e < E && gauss; ++e) {
            const int in = net.dims[L - 1], out = net.dims[L], IT = net.tiles[L - 1], OT = net.tiles[L];
            memcpy(h.data() + e * np + head.woff, head_w[e], sizeof(float) * in * out);
            memcpy(h.data() + e * np + head.boff, head_b[e], sizeof(float) * out);
            float* f = s.data() + e * slab + off_f[L];
            float* r = s.data() + e * slab + off_r[L];
            for (int i = 0; i < in; ++i)
                for (int o = 0; o < out; ++o) {
                    f[train_wf_index(IT, i, o)] = head_w[e][(size_t)i * out + o];
                    r[train_wr_index(OT, i, o)] = head_w[e][(size_t)i * out + o];
                }
            memcpy(s.data() + e * slab + off_b[L], head_b[e], sizeof(float) * out);
        }
        theta.alloc(h.size());
        m.alloc(h.size());
        v.alloc(h.size());
        pows.alloc((size_t)4 * E);
        packs.alloc(s.size());
        HIP_CHECK(hipMemcpy(theta.p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemset(m.p, 0, h.size() * sizeof(float)));
        HIP_CHECK(hipMemset(v.p, 0, h.size() * sizeof(float)));
        const std::vector<double> ones((size_t)4 * E, 1.0);
        HIP_CHECK(hipMemcpy(pows.p, ones.data(), ones.size() * sizeof(double), hipMemcpyHostToDevice));
        HIP_CHECK(hipMemcpy(packs.p, s.data(), s.size() * sizeof(float), hipMemcpyHostToDevice));
        for (int l = 0; l < L; ++l) {
            net.wf[l] = packs.p + off_f[l];
            net.wr[l] = packs.p + off_r[l];
            net.bp[l] = packs.p + off_b[l];
        }
        if (gauss) {
            const int O = net.dims[L];
            std::vector<float> b(lo, lo + O);
            b.insert(b.end(), hi, hi + O);
            lvb.alloc(b.size());
            HIP_CHECK(hipMemcpy(lvb.p, b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
            head.wf = packs.p + off_f[L];
            head.wr = packs.p + off_r[L];
            head.bp = packs.p + off_b[L];
            head.min_lv = lvb.p;
            head.max_lv = lvb.p + O;
        }
        const int bytes = net.lds_floats * 4;
        if (bytes > 64 * 1024) {
            for (const void* f : {reinterpret_cast<const void*>(k_train_fwd_bwd<false, false>), reinterpret_cast<const void*>(k_train_fwd_bwd<true, false>),
                                  reinterpret_cast<const void*>(k_train_forward_mse<false, false>),
                                  reinterpret_cast<const void*>(k_train_forward_mse<true, false>)})
                HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        }
        if (bytes > 64 * 1024 && gauss) {        // besides: residual_rms is the mean network's, through the head-less forward
            for (const void* f : {reinterpret_cast<const void*>(k_train_fwd_bwd<false, true>), reinterpret_cast<const void*>(k_train_fwd_bwd<true, true>),
                                  reinterpret_cast<const void*>(k_train_forward_mse<false, true>),
                                  reinterpret_cast<const void*>(k_train_forward_mse<true, true>)})
                HIP_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        }
    }
    ~Trainer() {
        if (stream) {
            (void)hipStreamSynchronize(stream);
            (void)hipStreamDestroy(stream);
        }
    }

    static void upload(DevBuf<float>& d, const float* h, size_t count) {
        d.alloc(count);
        if (count) HIP_CHECK(hipMemcpy(d.p, h, count * sizeof(float), hipMemcpyHostToDevice));
    }

    void set_data(const float* tin, const float* tout, int nt, const float* vi, const float* vo, int nv) {
        const int D = net.dims[0], O = net.dims[net.L];
        upload(din, tin, (size_t)nt * D);
        upload(dout, tout, (size_t)nt * O);
        upload(vin, vi, (size_t)nv * D);
        upload(vout, vo, (size_t)nv * O);
        n_train = nt;
        n_val = nv;
        has_data = true;
        member_rows.clear();                     // the rows of another dataset
    }

    void set_member_rows(const int32_t* rows) {
        REQUIRE(has_data, BBMPC_E_STATE, "trainer: bbmpc_trainer_set_member_rows before bbmpc_trainer_set_data");
        if (!rows) {
            member_rows.clear();
            return;
        }
        const size_t count = (size_t)E * n_train;
        for (size_t i = 0; i < count; ++i)
            REQUIRE(rows[i] >= 0 && rows[i] < n_train, BBMPC_E_INVALID, "trainer: a member row outside [0, n_train)");
        member_rows.assign(rows, rows + count);
    }

    // a single-member entry point on an ensemble
    void require_single(const char* call, const char* instead) const {
        REQUIRE(E == 1, BBMPC_E_STATE, std::string("trainer: ") + call + " on an ensemble of " + std::to_string(E) + " members; " + instead);
    }

    static void check_batch(int B) {
        REQUIRE(B >= 1 && B <= TR_MAX_BATCH, BBMPC_E_UNSUPPORTED, "trainer: batch_size must lie in [1, 4096]");
    }

    // forward + backward of every member's batch (member e: d_idx[e * idx_stride .. + B), device pointer) into part / lossp
    // stop: the early-stopping state the launch reads (mon.p + parity), null outside a monitored fit
    void launch_step(const int* d_idx, long long idx_stride, int B, const TrainMon* stop = nullptr) {
        TrainStepArgs q;
        q.n = net;
        q.din = din.p;
        q.dout = dout.p;
        q.idx = d_idx;
        q.idx_stride = idx_stride;
        q.row0 = 0;
        q.B = B;
        q.part = part.p;
        q.lossp = lossp.p;
        q.stop = stop;
        q.h = head;
        const int tiles = (B + TR_ROWS - 1) / TR_ROWS;
        const dim3 grid(tiles, E), block(net.nw * 64);
        const size_t lds = (size_t)net.lds_floats * 4;
        if (gauss) {
            if (stop) hipLaunchKernelGGL((k_train_fwd_bwd<true, true>), grid, block, lds, stream, q);
            else hipLaunchKernelGGL((k_train_fwd_bwd<false, true>), grid, block, lds, stream, q);
        } else if (stop) hipLaunchKernelGGL((k_train_fwd_bwd<true, false>), grid, block, lds, stream, q);
        else hipLaunchKernelGGL((k_train_fwd_bwd<false, false>), grid, block, lds, stream, q);
        HIP_CHECK(hipGetLastError());
    }

    // member e's loss goes to loss_slot[e * loss_stride]
    void launch_update(int rule_, int B, float* loss_slot, int loss_stride, float* grads_out, const TrainMon* stop = nullptr) {
        TrainUpdateArgs u;
        u.n = net;
        u.theta = theta.p;
        u.m = m.p;
        u.v = v.p;
        u.part = part.p;
        u.lossp = lossp.p;
        u.ntiles = (B + TR_ROWS - 1) / TR_ROWS;
        u.rule = rule_;
        const double b1 = 0.9, b2 = 0.999, rho = 0.9;          // Keras TF-2.0 defaults
        u.lr = (float)lr;
        u.b1 = (float)b1;
        u.b2 = (float)b2;
        u.omb1 = (float)(1.0 - b1);
        u.omb2 = (float)(1.0 - b2);
        u.rho = (float)rho;
        u.omrho = (float)(1.0 - rho);
        u.eps = 1e-7f;
        u.lr_d = lr;
        u.b1_d = b1;
        u.b2_d = b2;
        u.pows = pows.p;
        u.parity = (int)(steps & 1);
        u.inv_count = (float)(1.0 / ((double)B * net.dims[net.L]));
        u.gscale = (float)(2.0 / ((double)B * net.dims[net.L]));
        u.loss_acc = loss_slot;
        u.loss_stride = loss_stride;
        u.grads_out = grads_out;
        u.wd_on = 0;
        for (int l = 0; l < TR_MAX_LAYERS; ++l) {
            u.wd[l] = wd[l];
            u.lrwd[l] = u.lr * wd[l];
            u.wd_on |= wd[l] != 0.0f;
        }
        u.wd_mode = wd_mode;
        u.stop = stop;
        u.h = head;
        const dim3 grid((net.n_params + 255) / 256, E);
        if (gauss) {
            if (stop || u.wd_on) hipLaunchKernelGGL((k_train_update<true, true>), grid, dim3(256), 0, stream, u);
            else hipLaunchKernelGGL((k_train_update<false, true>), grid, dim3(256), 0, stream, u);
        } else if (stop || u.wd_on) hipLaunchKernelGGL((k_train_update<true, false>), grid, dim3(256), 0, stream, u);
        else hipLaunchKernelGGL((k_train_update<false, false>), grid, dim3(256), 0, stream, u);
        HIP_CHECK(hipGetLastError());
        if (rule_ != TR_RULE_NONE) ++steps;
    }

    void ensure_step_buffers(int B) {
        const size_t tiles = (size_t)(B + TR_ROWS - 1) / TR_ROWS;
        if (part.n < tiles * net.n_params * E) part.alloc(tiles * net.n_params * E);
        if (lossp.n < tiles * E) lossp.alloc(tiles * E);
    }

    // every member forward on the same rows: tile_loss [E][batches * tiles], colsq_out [E][batches * tiles][O]
    // nll: the Gaussian form (per tile the sum of wsq + lv); false on a Gaussian trainer: the mean network's squared errors
    void launch_mse(const float* in, const float* out, int batches, int B, float* tile_loss, float* colsq_out, const TrainMon* stop = nullptr,
                    bool nll = false) {
        TrainMseArgs q;
        q.n = net;
        q.din = in;
        q.dout = out;
        q.B = B;
        q.tiles_per_batch = (B + TR_ROWS - 1) / TR_ROWS;
        q.tile_loss = tile_loss;
        q.colsq = colsq_out;
        q.stop = stop;
        q.h = head;
        const dim3 grid((unsigned)((size_t)batches * q.tiles_per_batch), E), block(net.nw * 64);
        const size_t lds = (size_t)net.lds_floats * 4;
        if (nll) {
            if (stop) hipLaunchKernelGGL((k_train_forward_mse<true, true>), grid, block, lds, stream, q);
            else hipLaunchKernelGGL((k_train_forward_mse<false, true>), grid, block, lds, stream, q);
        } else if (stop) hipLaunchKernelGGL((k_train_forward_mse<true, false>), grid, block, lds, stream, q);
        else hipLaunchKernelGGL((k_train_forward_mse<false, false>), grid, block, lds, stream, q);
        HIP_CHECK(hipGetLastError());
    }

    // Every member `epochs` epochs.  perms_h: [E][epochs][n_train] or null (member e then draws from train_member_seed(seed,
    // e)); losses [E][epochs].  Batch rows of member e: member_rows[e][perm[e][epoch][pos + r]], composed here into one index
    // array [E][epochs][n_train].  index_bound: what E * epochs * n_train has to stay below.
    void fit(int epochs, int B, const int32_t* perms_h, uint64_t seed, float* train_loss, float* val_loss_out, long long index_bound) {
        REQUIRE(has_data, BBMPC_E_STATE, "trainer: a fit before bbmpc_trainer_set_data");
        REQUIRE(epochs >= 1, BBMPC_E_INVALID, "trainer: epochs must be >= 1");
        check_batch(B);
        const int n = n_train, nb = n / B, nvb = n_val / B;
        const int tpb = (B + TR_ROWS - 1) / TR_ROWS;
        const size_t en = (size_t)epochs * n;    // a member's stretch of the index array
        REQUIRE((long long)nvb * tpb < (1ll << 31), BBMPC_E_UNSUPPORTED, "trainer: dataset too large");
        REQUIRE((long long)E * epochs * n < index_bound, BBMPC_E_UNSUPPORTED,
                "trainer: dataset too large: n_members * epochs * n_train = " + std::to_string((long long)E * epochs * n) +
                    " index entries, the limit is below " + std::to_string(index_bound));
        const bool monitor = patience > 0 || restore_best;
        REQUIRE(!monitor || nvb > 0, BBMPC_E_STATE,
                "trainer: early stopping / restore_best need a validation loss, and n_val = " + std::to_string(n_val) +
                    " rows hold no full batch of " + std::to_string(B));
        std::vector<int32_t> composed;
        if (nb > 0) {
            if (perms_h)
                for (size_t i = 0; i < en * E; ++i)
                    REQUIRE(perms_h[i] >= 0 && perms_h[i] < n, BBMPC_E_INVALID, "trainer: a permutation entry outside [0, n_train)");
            if (!perms_h || !member_rows.empty()) {
                composed.resize(en * E);
                for (int e = 0; e < E; ++e) {
                    int32_t* dst = composed.data() + e * en;
                    if (perms_h) memcpy(dst, perms_h + e * en, en * sizeof(int32_t));
                    else
                        for (int k = 0; k < epochs; ++k) train_draw_permutation(train_member_seed(seed, e), k, n, dst + (size_t)k * n);
                    if (!member_rows.empty()) {
                        const int32_t* rows = member_rows.data() + (size_t)e * n;
                        for (size_t i = 0; i < en; ++i) dst[i] = rows[dst[i]];
                    }
                }
                perms_h = composed.data();
            }
            ensure_step_buffers(B);
            if (perms.n < en * E) perms.alloc(en * E);
            HIP_CHECK(hipMemcpy(perms.p, perms_h, en * E * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        const size_t nl = (size_t)epochs * E;
        if (loss_acc.n < nl) { loss_acc.alloc(nl); val_loss.alloc(nl); }
        HIP_CHECK(hipMemsetAsync(loss_acc.p, 0, nl * sizeof(float), stream));
        if (nvb > 0) {
            if (val_tiles.n < (size_t)nvb * tpb * E) val_tiles.alloc((size_t)nvb * tpb * E);
            if (val_batch.n < (size_t)nvb * E) val_batch.alloc((size_t)nvb * E);
        }
        const float nan = std::numeric_limits<float>::quiet_NaN();
        if (monitor) {
            if (mon.n < (size_t)2 * E) mon.alloc((size_t)2 * E);
            if (restore_best && best_theta.n < (size_t)net.n_params * E) best_theta.alloc((size_t)net.n_params * E);
            mon_host.assign((size_t)2 * E, TrainMon{std::numeric_limits<float>::infinity(), -1, 0, 0});
            HIP_CHECK(hipMemcpyAsync(mon.p, mon_host.data(), mon_host.size() * sizeof(TrainMon), hipMemcpyHostToDevice, stream));
        }
        // the epochs: nothing but launches on one stream, each for all members.  Every epoch is enqueued whatever the monitor
        // will decide: a stopped member's workgroups return at once.
        for (int k = 0; k < epochs; ++k) {
            const TrainMon* stop = monitor ? mon.p + (k & 1) : nullptr;
            for (int bi = 0; bi < nb; ++bi) {
                launch_step(perms.p + (size_t)k * n + (size_t)bi * B, (long long)en, B, stop);
                launch_update(rule, B, loss_acc.p + k, epochs, nullptr, stop);
            }
            if (nvb > 0) {
                launch_mse(vin.p, vout.p, nvb, B, val_tiles.p, nullptr, stop, gauss);
                hipLaunchKernelGGL(k_train_val_reduce, dim3(1, E), dim3(256), 0, stream, (const float*)val_tiles.p, nvb, tpb,
                                   (float)(1.0 / ((double)B * net.dims[net.L])), val_batch.p, val_loss.p + k, epochs, stop);
                HIP_CHECK(hipGetLastError());
            }
            if (monitor) {
                hipLaunchKernelGGL(k_train_monitor, dim3(restore_best ? (net.n_params + 255) / 256 : 1, E), dim3(256), 0, stream, mon.p,
                                   (const float*)val_loss.p + k, epochs, k, patience, min_delta, (const float*)theta.p,
                                   restore_best ? best_theta.p : (float*)nullptr, net.n_params);
                HIP_CHECK(hipGetLastError());
            }
        }
        if (restore_best) {
            const dim3 grid((net.n_params + 255) / 256, E);
            const TrainMon* last = mon.p + (epochs & 1);
            if (gauss) hipLaunchKernelGGL(k_train_restore<true>, grid, dim3(256), 0, stream, net, last, (const float*)best_theta.p, theta.p, head);
            else hipLaunchKernelGGL(k_train_restore<false>, grid, dim3(256), 0, stream, net, last, (const float*)best_theta.p, theta.p, head);
            HIP_CHECK(hipGetLastError());
        }
        std::vector<float> tl(nl), vl(nl);
        HIP_CHECK(hipMemcpyAsync(tl.data(), loss_acc.p, nl * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (nvb > 0) HIP_CHECK(hipMemcpyAsync(vl.data(), val_loss.p, nl * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (monitor) HIP_CHECK(hipMemcpyAsync(mon_host.data(), mon.p, mon_host.size() * sizeof(TrainMon), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        // the report: without monitoring every member ran every epoch and nothing was tracked
        rep_epochs.assign(E, epochs);
        rep_best_epoch.assign(E, -1);
        rep_best_val.assign(E, nan);
        for (int e = 0; e < E && monitor; ++e) {
            const TrainMon& s = mon_host[(size_t)2 * e + (epochs & 1)];
            if (s.stopped) rep_epochs[e] = s.stopped;
            rep_best_epoch[e] = s.best_epoch;
            if (s.best_epoch >= 0) rep_best_val[e] = s.best;
        }
        for (size_t i = 0; i < nl; ++i) {
            const bool ran = (int)(i % epochs) < rep_epochs[i / epochs];       // a stopped member's later epochs: NaN
            train_loss[i] = nb > 0 && ran ? (float)((double)tl[i] / nb) : nan;
            val_loss_out[i] = nvb > 0 && ran ? vl[i] : nan;
        }
    }

    void set_weight_decay(const float* decay, int mode) {
        REQUIRE(mode == TR_DECAY_L2 || mode == TR_DECAY_DECOUPLED, BBMPC_E_INVALID,
                "trainer: unknown weight decay mode " + std::to_string(mode) + " (BBMPC_TRAIN_DECAY_L2 or BBMPC_TRAIN_DECAY_DECOUPLED)");
        for (int l = 0; decay && l < net.L; ++l)
            REQUIRE(std::isfinite(decay[l]) && decay[l] >= 0.0f, BBMPC_E_INVALID,
                    "trainer: weight decay of layer " + std::to_string(l) + " must be finite and >= 0");
        for (int l = 0; l < TR_MAX_LAYERS; ++l) wd[l] = decay && l < net.L ? decay[l] : 0.0f;
        wd_mode = mode;
    }

    void set_early_stopping(int patience_, float min_delta_, int restore) {
        REQUIRE(patience_ >= 0, BBMPC_E_INVALID, "trainer: patience must be >= 0 (0: no early stopping)");
        REQUIRE(std::isfinite(min_delta_) && min_delta_ >= 0.0f, BBMPC_E_INVALID, "trainer: min_delta must be finite and >= 0");
        patience = patience_;
        min_delta = min_delta_;
        restore_best = restore != 0;
    }

    void get_fit_report(int32_t* epochs_run, int32_t* best_epoch, float* best_val) const {
        REQUIRE(!rep_epochs.empty(), BBMPC_E_STATE, "trainer: bbmpc_trainer_get_fit_report before any fit");
        memcpy(epochs_run, rep_epochs.data(), sizeof(int32_t) * E);
        memcpy(best_epoch, rep_best_epoch.data(), sizeof(int32_t) * E);
        memcpy(best_val, rep_best_val.data(), sizeof(float) * E);
    }

    void gradients(const int32_t* idx_h, int B, float* grads_out, float* loss_out) {
        REQUIRE(has_data, BBMPC_E_STATE, "trainer: bbmpc_trainer_gradients before bbmpc_trainer_set_data");
        check_batch(B);
        for (int i = 0; i < B; ++i) REQUIRE(idx_h[i] >= 0 && idx_h[i] < n_train, BBMPC_E_INVALID, "trainer: a row index outside [0, n_train)");
        ensure_step_buffers(B);
        if (idx.n < (size_t)B) idx.alloc(B);
        if (grads.n < (size_t)net.n_params + 1) grads.alloc((size_t)net.n_params + 1);
        HIP_CHECK(hipMemcpy(idx.p, idx_h, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
        launch_step(idx.p, 0, B);
        launch_update(TR_RULE_NONE, B, grads.p + net.n_params, 0, grads.p);
        std::vector<float> h((size_t)net.n_params + 1);
        HIP_CHECK(hipMemcpyAsync(h.data(), grads.p, h.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        memcpy(grads_out, h.data(), (size_t)net.n_params * sizeof(float));
        *loss_out = h[net.n_params];
    }

    void get_params(int member, float* const* weights, float* const* biases) {
        std::vector<float> h((size_t)net.n_params);
        HIP_CHECK(hipMemcpyAsync(h.data(), theta.p + (size_t)member * net.n_params, h.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        for (int l = 0; l < net.L; ++l) {
            memcpy(weights[l], h.data() + net.woff[l], sizeof(float) * net.dims[l] * net.dims[l + 1]);
            memcpy(biases[l], h.data() + net.boff[l], sizeof(float) * net.dims[l + 1]);
        }
    }

    void get_logvar_head(int member, float* w_out, float* b_out) {
        const size_t count = (size_t)net.n_params - head.woff;     // W_v, then b_v
        std::vector<float> h(count);
        HIP_CHECK(hipMemcpyAsync(h.data(), theta.p + (size_t)member * net.n_params + head.woff, count * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        memcpy(w_out, h.data(), sizeof(float) * (head.boff - head.woff));
        memcpy(b_out, h.data() + (head.boff - head.woff), sizeof(float) * net.dims[net.L]);
    }

    // rms_out [E][O]: every member on the same n rows, uploaded once
    void residual_rms(const float* in, const float* out, int n, float* rms_out) {
        REQUIRE(n >= 1, BBMPC_E_INVALID, "trainer: residual_rms needs at least one row");
        const int D = net.dims[0], O = net.dims[net.L];
        const int tiles = (n + TR_ROWS - 1) / TR_ROWS;
        upload(rin, in, (size_t)n * D);
        upload(rout, out, (size_t)n * O);
        if (colsq.n < (size_t)tiles * O * E) colsq.alloc((size_t)tiles * O * E);
        if (rms.n < (size_t)O * E) rms.alloc((size_t)O * E);
        launch_mse(rin.p, rout.p, 1, n, nullptr, colsq.p);
        hipLaunchKernelGGL(k_train_rms_reduce, dim3((O + 63) / 64, E), dim3(64), 0, stream, (const float*)colsq.p, tiles, O, (float)(1.0 / n), rms.p);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(rms_out, rms.p, (size_t)O * E * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
    }
};

}  // namespace bbmpc

using bbmpc::Trainer;
using bbmpc::TrainNet;

struct bbmpc_trainer_s {
    Trainer* t;
};

#define CHECK_TRAINER(h)                                                       \
    if (!(h) || !(h)->t) throw HipError(BBMPC_E_INVALID, "null trainer");      \
    DeviceGuard _device_guard((h)->t->device)

// what bbmpc_trainer_create and bbmpc_trainer_create_ensemble share; every refusal comes before a device is touched
// gaussian: with a log-variance head (head_weights / head_biases [n_members], the bounds [dims[n_layers]])
static void trainer_create(bbmpc_trainer* out, int32_t device, int32_t n_members, int32_t n_layers, const int32_t* dims,
                           const int32_t* activations, const float* const* weights, const float* const* biases, int32_t rule,
                           float learning_rate, bool gaussian = false, const float* const* head_weights = nullptr,
                           const float* const* head_biases = nullptr, const float* min_logvar = nullptr, const float* max_logvar = nullptr) {
    REQUIRE(out, BBMPC_E_INVALID, "trainer: null output handle");
    *out = nullptr;
    REQUIRE(n_members >= 1 && n_members <= bbmpc::TR_MAX_MEMBERS, BBMPC_E_UNSUPPORTED,
            "trainer: n_members must lie in [1, 8] (BBMPC_MAX_ENSEMBLE_MEMBERS)");
    TrainNet n;
    bbmpc::TrainHead head;
    bbmpc::train_describe(n, n_layers, dims, activations);
    if (gaussian) bbmpc::train_describe_head(n, head);
    REQUIRE(weights && biases, BBMPC_E_INVALID, "trainer: null weights / biases");
    for (int i = 0; i < n_members * n_layers; ++i) REQUIRE(weights[i] && biases[i], BBMPC_E_INVALID, "trainer: a null weight or bias array");
    if (gaussian) {
        REQUIRE(head_weights && head_biases, BBMPC_E_INVALID, "trainer: null head_weights / head_biases");
        for (int e = 0; e < n_members; ++e)
            REQUIRE(head_weights[e] && head_biases[e], BBMPC_E_INVALID, "trainer: a null log-variance head kernel or bias array");
        bbmpc::train_check_logvar_bounds(min_logvar, max_logvar, n.dims[n.L]);
    }
    REQUIRE(rule == BBMPC_TRAIN_ADAM || rule == BBMPC_TRAIN_SGD || rule == BBMPC_TRAIN_RMSPROP, BBMPC_E_INVALID, "trainer: unknown update rule");
    REQUIRE(std::isfinite(learning_rate) && learning_rate > 0.0f, BBMPC_E_INVALID, "trainer: learning_rate must be finite and positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        throw HipError(BBMPC_E_NO_DEVICE, "no HIP device available: this library has no CPU fallback");
    REQUIRE(device < ndev, BBMPC_E_NO_DEVICE, "trainer: device out of range");
    int dev = device;
    if (dev < 0) HIP_CHECK(hipGetDevice(&dev));
    DeviceGuard guard(dev);
    Trainer* t = new Trainer(n, dev, n_members, weights, biases, rule, (double)learning_rate, gaussian ? &head : nullptr, head_weights,
                             head_biases, min_logvar, max_logvar);
    *out = new bbmpc_trainer_s{t};
}

// what bbmpc_trainer_lds_bytes and bbmpc_trainer_lds_bytes_gaussian share
static int64_t trainer_lds_bytes(int32_t n_layers, const int32_t* dims, const int32_t* activations, bool gaussian) {
    REQUIRE(n_layers >= 1 && n_layers <= bbmpc::TR_MAX_LAYERS && dims && activations, BBMPC_E_INVALID, "trainer: n_layers outside [1, 8] or null arrays");
    TrainNet n;
    memset(&n, 0, sizeof(n));
    n.L = n_layers;
    for (int l = 0; l <= n_layers; ++l) {
        REQUIRE(dims[l] >= 1, BBMPC_E_INVALID, "trainer: a layer width < 1");
        n.dims[l] = dims[l];
    }
    for (int l = 0; l < n_layers; ++l) n.act[l] = activations[l];
    bbmpc::train_lds_layout(n);
    if (gaussian) {
        bbmpc::TrainHead head;
        bbmpc::train_lds_layout_head(n, head);
    }
    return (int64_t)n.lds_floats * 4;
}

extern "C" {

int bbmpc_trainer_lds_bytes(int32_t n_layers, const int32_t* dims, const int32_t* activations, int64_t* bytes) {
    API_BEGIN
    CHECK_PTR(bytes);
    *bytes = 0;
    *bytes = trainer_lds_bytes(n_layers, dims, activations, false);
    API_END
}

int bbmpc_trainer_lds_bytes_gaussian(int32_t n_layers, const int32_t* dims, const int32_t* activations, int64_t* bytes) {
    API_BEGIN
    CHECK_PTR(bytes);
    *bytes = 0;
    *bytes = trainer_lds_bytes(n_layers, dims, activations, true);
    API_END
}

int bbmpc_trainer_create_gaussian(bbmpc_trainer* out, int32_t device, int32_t n_members, int32_t n_layers, const int32_t* dims,
                                  const int32_t* activations, const float* const* weights, const float* const* biases,
                                  const float* const* head_weights, const float* const* head_biases, const float* min_logvar,
                                  const float* max_logvar, int32_t rule, float learning_rate) {
    API_BEGIN
    trainer_create(out, device, n_members, n_layers, dims, activations, weights, biases, rule, learning_rate, true, head_weights, head_biases,
                   min_logvar, max_logvar);
    API_END
}

int bbmpc_trainer_get_logvar_head(bbmpc_trainer t, int32_t member, float* head_weights_out, float* head_bias_out) {
    API_BEGIN
    CHECK_TRAINER(t);
    REQUIRE(t->t->gauss, BBMPC_E_STATE, "trainer: bbmpc_trainer_get_logvar_head on a trainer without a log-variance head (bbmpc_trainer_create_gaussian makes one)");
    REQUIRE(head_weights_out && head_bias_out, BBMPC_E_INVALID, "trainer: null log-variance head outputs");
    REQUIRE(member >= 0 && member < t->t->E, BBMPC_E_INVALID, "trainer: member outside [0, n_members)");
    t->t->get_logvar_head(member, head_weights_out, head_bias_out);
    API_END
}

int bbmpc_trainer_create(bbmpc_trainer* out, int32_t device, int32_t n_layers, const int32_t* dims, const int32_t* activations,
                         const float* const* weights, const float* const* biases, int32_t rule, float learning_rate) {
    API_BEGIN
    trainer_create(out, device, 1, n_layers, dims, activations, weights, biases, rule, learning_rate);
    API_END
}

int bbmpc_trainer_create_ensemble(bbmpc_trainer* out, int32_t device, int32_t n_members, int32_t n_layers, const int32_t* dims,
                                  const int32_t* activations, const float* const* weights, const float* const* biases, int32_t rule,
                                  float learning_rate) {
    API_BEGIN
    trainer_create(out, device, n_members, n_layers, dims, activations, weights, biases, rule, learning_rate);
    API_END
}

int bbmpc_trainer_destroy(bbmpc_trainer t) {
    API_BEGIN
    if (t) {
        if (t->t) {
            DeviceGuard g(t->t->device);
            delete t->t;
        }
        delete t;
    }
    API_END
}

int bbmpc_trainer_set_data(bbmpc_trainer t, const float* train_in, const float* train_out, int32_t n_train, const float* val_in,
                           const float* val_out, int32_t n_val) {
    API_BEGIN
    CHECK_TRAINER(t);
    REQUIRE(n_train >= 0 && n_val >= 0, BBMPC_E_INVALID, "trainer: negative row count");
    REQUIRE(n_train == 0 || (train_in && train_out), BBMPC_E_INVALID, "trainer: null training rows");
    REQUIRE(n_val == 0 || (val_in && val_out), BBMPC_E_INVALID, "trainer: null validation rows");
    t->t->set_data(train_in, train_out, n_train, val_in, val_out, n_val);
    API_END
}

int bbmpc_trainer_set_member_rows(bbmpc_trainer t, const int32_t* rows) {
    API_BEGIN
    CHECK_TRAINER(t);
    t->t->set_member_rows(rows);
    API_END
}

int bbmpc_trainer_fit(bbmpc_trainer t, int32_t epochs, int32_t batch_size, const int32_t* perms, uint64_t seed, float* train_loss_out,
                      float* val_loss_out) {
    API_BEGIN
    CHECK_TRAINER(t);
    CHECK_PTR(train_loss_out);
    CHECK_PTR(val_loss_out);
    t->t->require_single("bbmpc_trainer_fit", "call bbmpc_trainer_fit_ensemble");
    t->t->fit(epochs, batch_size, perms, seed, train_loss_out, val_loss_out, 1ll << 40);
    API_END
}

int bbmpc_trainer_fit_ensemble(bbmpc_trainer t, int32_t epochs, int32_t batch_size, const int32_t* perms, uint64_t seed,
                               float* train_loss_out, float* val_loss_out) {
    API_BEGIN
    CHECK_TRAINER(t);
    REQUIRE(train_loss_out && val_loss_out, BBMPC_E_INVALID, "trainer: null loss outputs");
    t->t->fit(epochs, batch_size, perms, seed, train_loss_out, val_loss_out, 1ll << 31);
    API_END
}

int bbmpc_trainer_get_params(bbmpc_trainer t, float* const* weights, float* const* biases) {
    API_BEGIN
    CHECK_TRAINER(t);
    CHECK_PTR(weights);
    CHECK_PTR(biases);
    t->t->require_single("bbmpc_trainer_get_params", "call bbmpc_trainer_get_member_params");
    for (int l = 0; l < t->t->net.L; ++l) REQUIRE(weights[l] && biases[l], BBMPC_E_INVALID, "trainer: a null weight or bias array");
    t->t->get_params(0, weights, biases);
    API_END
}

int bbmpc_trainer_get_member_params(bbmpc_trainer t, int32_t member, float* const* weights, float* const* biases) {
    API_BEGIN
    CHECK_TRAINER(t);
    REQUIRE(weights && biases, BBMPC_E_INVALID, "trainer: null weights / biases");
    REQUIRE(member >= 0 && member < t->t->E, BBMPC_E_INVALID, "trainer: member outside [0, n_members)");
    for (int l = 0; l < t->t->net.L; ++l) REQUIRE(weights[l] && biases[l], BBMPC_E_INVALID, "trainer: a null weight or bias array");
    t->t->get_params(member, weights, biases);
    API_END
}

int bbmpc_trainer_residual_rms(bbmpc_trainer t, const float* in, const float* out, int32_t n, float* rms_out) {
    API_BEGIN
    CHECK_TRAINER(t);
    CHECK_PTR(in);
    CHECK_PTR(out);
    CHECK_PTR(rms_out);
    t->t->require_single("bbmpc_trainer_residual_rms", "call bbmpc_trainer_residual_rms_ensemble");
    t->t->residual_rms(in, out, n, rms_out);
    API_END
}

int bbmpc_trainer_residual_rms_ensemble(bbmpc_trainer t, const float* in, const float* out, int32_t n, float* rms_out) {
    API_BEGIN
    CHECK_TRAINER(t);
    REQUIRE(in && out && rms_out, BBMPC_E_INVALID, "trainer: null rows or output");
    t->t->residual_rms(in, out, n, rms_out);
    API_END
}

int bbmpc_trainer_gradients(bbmpc_trainer t, const int32_t* idx, int32_t batch_size, float* grads_out, float* loss_out) {
    API_BEGIN
    CHECK_TRAINER(t);
    CHECK_PTR(idx);
    CHECK_PTR(grads_out);
    CHECK_PTR(loss_out);
    t->t->require_single("bbmpc_trainer_gradients", "it is the single trainer's test window (bbmpc_trainer_fit_ensemble fits an ensemble)");
    t->t->gradients(idx, batch_size, grads_out, loss_out);
    API_END
}

int bbmpc_trainer_set_weight_decay(bbmpc_trainer t, const float* decay, int32_t mode) {
    API_BEGIN
    CHECK_TRAINER(t);
    t->t->set_weight_decay(decay, mode);
    API_END
}

int bbmpc_trainer_set_early_stopping(bbmpc_trainer t, int32_t patience, float min_delta, int32_t restore_best) {
    API_BEGIN
    CHECK_TRAINER(t);
    t->t->set_early_stopping(patience, min_delta, restore_best);
    API_END
}

int bbmpc_trainer_get_fit_report(bbmpc_trainer t, int32_t* epochs_run, int32_t* best_epoch, float* best_val) {
    API_BEGIN
    CHECK_TRAINER(t);
    REQUIRE(epochs_run && best_epoch && best_val, BBMPC_E_INVALID, "trainer: null report outputs");
    t->t->get_fit_report(epochs_run, best_epoch, best_val);
    API_END
}

}  // extern "C"
