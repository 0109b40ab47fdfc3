// Training a Dense stack on the matrix cores (bbmpc_trainer_*): mini-batch MSE, backprop and the
// Keras TF-2.0 update rules (adam / sgd / rmsprop) of dynamics_functions/_train_torch.DenseTrainer, as three kernels.
//
//   k_train_fwd_bwd      grid ceil(B / 16): a workgroup owns 16 rows of the batch.  It gathers them through the epoch's
//                        permutation, runs the forward stack with EVERY layer's output tile resident in LDS, forms
//                        delta_{L-1} = act'(y_L) * (y_L - t) -- the factor 2 / (B O) is left to k_train_update, which
//                        applies it ONCE to each summed gradient element -- and sweeps backwards: per layer its share of
//                        dW_l = y_l^T delta_l (an MFMA product whose K extent is the tile's 16 rows), of
//                        db_l = column sums of delta_l in row order, and g = delta_l W_l^T for the layer below.  Shares go
//                        to part[tile][n_params], the tile's sum of squared errors to lossp[tile].  No atomics.
//   k_train_update       one lane per parameter: adds the shares in ascending tile order, scales the sum by 2 / (B O)
//                        (the only rounding of a gradient whose terms are exact, e.g. small integers; where B O is a
//                        power of two the bits are those of scaling every delta), applies the rule (m, v and the
//                        running powers b1^t, b2^t live on the device, the powers in double) and writes the parameter in
//                        every layout the step kernel reads: the operand pack of W, the pack of W^T, the padded bias.
//   k_train_forward_mse  forward only: per tile the squared error per output column and its sum (validation batches,
//                        residual_rms).
//
// Every product is v_mfma_f32_16x16x4_f32 (fp32 in, fp32 accumulate).  Layer tiles use kernels_mlp.hpp's layout: a tile
// array [T][64][4], lane l of tile t holding features 16 t + 4 (l >> 4) + {0..3} of row l & 15 -- the D fragment of one
// product is the B operand of the next, in both sweeps.  Operand packs are mlp_pack_layer's [OT][IT][64][4]: lane l, slot s
// of (ot, it) is M[16 it + 4 (l >> 4) + s][16 ot + (l & 15)], M = W for the forward sweep and W^T for the backward one,
// zero where an index passes the matrix.
//
// delta_l overwrites y_{l+1} in place (y_{l+1} is dead once act' is taken and dW_{l+1} is out), so the backward sweep
// needs ONE scratch tile array for g.  A layer's pre-activation is kept only for the codes whose derivative cannot be
// rebuilt from the output (train_needs_pre: swish); the others use DenseTrainer's forms in y.
//
// Rows >= B of the last tile are never read from the dataset, and their delta is set to zero in every layer: their
// shares are exact zeros.  Nothing depends on timing or on the grid: equal calls give equal bits.
//
// Members.  Every kernel has a second grid dimension, blockIdx.y = e < E <= TR_MAX_MEMBERS: the members of an ensemble are
// equally shaped networks fitted side by side.  A pointer below addresses member 0; member e's copy lies e member strides
// further (TrainNet::pstride for the operand packs, n_params for theta / m / v / a gradient, the grid's x extent for the
// share and loss buffers, the strides the argument structs name for the rest).  The dataset is shared; a member's own rows
// are an index map (TrainStepArgs::idx).  e is uniform over the workgroup, so the offsets are scalar arithmetic.  A member
// reads and writes nothing of another's and its arithmetic does not see E: E = 1 is the single trainer, bit for bit.
//
// Weight decay, early stopping, best-weights restore.
//   decay      k_train_update takes one lambda per layer and a mode by value; kernels only, never biases.  w0 is the value
//              before the step, g the data gradient (2 / (B O) applied), every line one float32 operation:
//                TR_DECAY_L2         g' = fma(lambda, w0, g), then the rule on g' exactly as on g
//                TR_DECAY_DECOUPLED  w1 = the rule's result on g, then w = fma(-(lr lambda), w0, w1), lr lambda rounded to
//                                    float32 once on the host; lr is the base rate, not Adam's lr_t
//              Both lines sit behind `lambda != 0`: a zero decay adds no operation to the value chain.  The kernel has
//              always found a parameter's layer to write the layouts; with a decay on, that lookup moves in front of the rule.
//   monitor    k_train_monitor, one launch per epoch behind k_train_val_reduce, grid (ceil(n_params / 256), E).  A member's
//              state (TrainMon: best, best_epoch, wait, stopped) is carried the way the Adam powers are: epoch k reads
//              mon[e][k & 1] and writes mon[e][~k & 1].  Every workgroup of the launch therefore takes its decision from
//              words no workgroup of the launch writes -- the decision is identical in all of them without a second launch
//              (decision, then copy) per epoch, and launches are what this trainer's time is made of.  On an improvement
//              the workgroups copy theta[e] to best_theta[e].  A stopped member's state is carried forward unchanged.
//   early exit k_train_fwd_bwd, k_train_update, k_train_forward_mse and k_train_val_reduce are given the state epoch k reads
//              (null: no monitoring) and return at once for a stopped member: uniform over the workgroup, nothing else
//              touched -- but for the Adam powers, which a stopped member's k_train_update hands from [parity] to
//              [parity ^ 1] unmultiplied, so that its step count stays its own when the trainer is fitted again.
//   restore    k_train_restore, grid (ceil(n_params / 256), E), once at the end of a fit: best_theta -> theta and every
//              layout the step kernel reads, for the members whose best_epoch >= 0.
//
// Log-variance head, Gaussian NLL: the NLL instantiations, a second template bool next to MON / REG.
// The head-less instantiations carry no test of it and are the code they were.
//   parameters theta = W_0 .. W_{L-1}, b_0 .. b_{L-1}, W_v [dims[L-1]][O], b_v [O]: DenseTrainer.params' order, every
//              head-less offset as it was.  The head's W pack, W^T pack and padded bias close the member's slab (TrainHead).
//   forward    in the last layer the head's tile product z = h W_v + b_v runs next to the mean's, on the same input tiles,
//              into a tile array of its own (TrainHead::zoff, T_L tiles between the adjoint scratch and the row / loss words).
//   elementwise, per valid element (tr_logvar; accurate expf / log1pf, the stage touches B O values per step):
//                lv1 = max_lv - softplus(max_lv - z);  lv = min_lv + softplus(lv1 - min_lv);  inv = exp(-lv)
//                diff = mu - t;  wsq = diff diff inv;  the thread's loss word += wsq + lv
//                delta_mu = act'(mu) (diff inv)                                        in place of y_L
//                delta_z  = 0.5 (1 - wsq) sigmoid(lv1 - min_lv) sigmoid(max_lv - z)    in place of z
//              The factor 0.5 is exact and lets k_train_update keep its ONE 2 / (B O) scaling of every summed gradient:
//              d loss / d z = (1 - wsq) dlv/dz / (B O).
//   backward   at layer L - 1: dW_v = h^T delta_z and db_v exactly as dW_{L-1} and db_{L-1}; g = delta_mu W_{L-1}^T +
//              delta_z W_v^T is ONE accumulator per output tile -- the mean's k tiles first, ascending, then the head's,
//              ascending (two tr_tile_product calls on the same acc).  Below that layer nothing changes.
//   update     W_v decays with the last layer's lambda, b_v never; snapshot and restore cover the head (n_params does).
//   validation k_train_forward_mse<., true> writes per tile the sum of wsq + lv: k_train_val_reduce and k_train_monitor work
//              on the NLL unchanged.  residual_rms stays the mean network's, through the head-less forward.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "activations_grad.hpp"

namespace bbmpc {

typedef float tr_f32x4 __attribute__((ext_vector_type(4)));

constexpr int TR_MAX_LAYERS = 8;
constexpr int TR_MAX_WIDTH = 512;
constexpr int TR_MAX_BATCH = 4096;
constexpr int TR_MAX_MEMBERS = 8;                   // BBMPC_MAX_ENSEMBLE_MEMBERS
constexpr int TR_ROWS = 16;                      // batch rows per workgroup
constexpr int TR_LDS_LIMIT = 159 * 1024;         // bytes, as the other kernels' carves
constexpr int TR_SCRATCH = 64 + 1024;            // floats: 16 row indices (padded to 64) + one word per thread
constexpr int TR_RULE_NONE = 0, TR_RULE_ADAM = 1, TR_RULE_SGD = 2, TR_RULE_RMSPROP = 3;      // BBMPC_TRAIN_*
constexpr int TR_DECAY_L2 = 0, TR_DECAY_DECOUPLED = 1;                                        // BBMPC_TRAIN_DECAY_*

// A member's early-stopping state, [E][2]: the epoch-k launches read [k & 1], k_train_monitor writes [~k & 1].
struct TrainMon {
    float best;                                  // the best validation loss so far; +inf before the first improvement
    int best_epoch;                              // its epoch; -1 before
    int wait;                                    // epochs since
    int stopped;                                 // 0: running; else the number of epochs the member ran
};

// activations whose derivative needs the pre-activation (act_grad's x): the forward sweep keeps that tile
__host__ __device__ inline bool train_needs_pre(int act) { return act == ACT_SWISH; }

// The network as the kernels see it.  theta is the parameter vector in natural order: W_0 .. W_{L-1} ([in][out] row
// major), then b_0 .. b_{L-1}; woff / boff index it (and m, v, a gradient, a row of the share buffer).
struct TrainNet {
    int L;
    int dims[TR_MAX_LAYERS + 1];
    int tiles[TR_MAX_LAYERS + 1];                // ceil(dims / 16)
    int act[TR_MAX_LAYERS];
    int woff[TR_MAX_LAYERS], boff[TR_MAX_LAYERS];
    int n_params;
    int yoff[TR_MAX_LAYERS + 1];                 // LDS offsets (floats) of y_0 .. y_L
    int zoff[TR_MAX_LAYERS];                     // ... of layer l's pre-activation, -1 when not kept
    int goff, soff;                              // the adjoint scratch [Tmax][64][4]; TR_SCRATCH floats
    int lds_floats;
    int nw;                                      // waves per workgroup
    float* wf[TR_MAX_LAYERS];                    // operand pack of W_l   [T_{l+1}][T_l][64][4]
    float* wr[TR_MAX_LAYERS];                    // operand pack of W_l^T [T_l][T_{l+1}][64][4]
    float* bp[TR_MAX_LAYERS];                    // b_l padded with zeros to 16 T_{l+1}
    int pstride;                                 // floats from member e's wf / wr / bp to member e + 1's (one slab per member)
};

// LDS carve in floats:  256 * (sum_{l=0..L} T_l  +  sum over swish layers of T_{l+1}  +  max_l T_l) + TR_SCRATCH,
// T_l = ceil(dims[l] / 16): the resident layer tiles, the kept pre-activations, the adjoint scratch, the row / loss words.
__host__ __device__ inline void train_lds_layout(TrainNet& n) {
    int o = 0, tmax = 1;
    for (int l = 0; l <= n.L; ++l) {
        n.tiles[l] = (n.dims[l] + 15) / 16;
        n.yoff[l] = o;
        o += n.tiles[l] * 256;
        tmax = tmax > n.tiles[l] ? tmax : n.tiles[l];
    }
    for (int l = 0; l < n.L; ++l) {
        n.zoff[l] = -1;
        if (train_needs_pre(n.act[l])) {
            n.zoff[l] = o;
            o += n.tiles[l + 1] * 256;
        }
    }
    n.goff = o; o += tmax * 256;
    n.soff = o; o += TR_SCRATCH;
    n.lds_floats = o;
    n.nw = tmax < 4 ? 4 : (tmax > 16 ? 16 : tmax);
}

// The log-variance head of a Gaussian trainer: a second last Dense layer on y_{L-1}, linear, with
// fixed per-output bounds.  It closes every argument struct, behind what the head-less kernels read.
struct TrainHead {
    int woff, boff;                              // theta offsets of W_v [dims[L-1]][O] and b_v [O]: behind b_{L-1}
    int zoff;                                    // LDS offset (floats) of the head's tile array [T_L][64][4]
    int pad_;
    float* wf;                                   // operand pack of W_v   [T_L][T_{L-1}][64][4]; member e's: + e * pstride
    float* wr;                                   // operand pack of W_v^T [T_{L-1}][T_L][64][4]
    float* bp;                                   // b_v padded with zeros to 16 T_L
    const float* min_lv;                         // [O], shared by the members
    const float* max_lv;
};

// The Gaussian carve: train_lds_layout's with T_L more tiles, the head's z, between the adjoint scratch and the words:
// 256 * (sum_l T_l + swish pre-activations + max_l T_l + T_L) + TR_SCRATCH floats.  Call after train_lds_layout.
__host__ __device__ inline void train_lds_layout_head(TrainNet& n, TrainHead& h) {
    h.zoff = n.soff;
    n.soff += n.tiles[n.L] * 256;
    n.lds_floats += n.tiles[n.L] * 256;
}

// offsets of parameter (i, o) of layer l in the two packs
__host__ __device__ inline size_t train_wf_index(int IT, int i, int o) {
    return (((size_t)(o >> 4) * IT + (i >> 4)) * 64 + (((i & 15) >> 2) * 16 + (o & 15))) * 4 + (i & 3);
}
__host__ __device__ inline size_t train_wr_index(int OT, int i, int o) {      // W^T: input o, output i
    return (((size_t)(i >> 4) * OT + (o >> 4)) * 64 + (((o & 15) >> 2) * 16 + (i & 15))) * 4 + (o & 3);
}

// The epoch permutations bbmpc_trainer_fit draws when it is given none: Fisher-Yates from the top, j = floor(u (i + 1) /
// 2^64) with u the next output of splitmix64, whose state starts at seed ^ (0xD1B54A32D192ED03 * (epoch + 1)).
inline uint64_t train_splitmix64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline void train_draw_permutation(uint64_t seed, int epoch, int n, int32_t* out) {
    uint64_t s = seed ^ (0xD1B54A32D192ED03ull * (uint64_t)(epoch + 1));
    for (int i = 0; i < n; ++i) out[i] = i;
    for (int i = n - 1; i >= 1; --i) {
        const uint64_t u = train_splitmix64(s);
        const int j = (int)(uint64_t)(((unsigned __int128)u * (uint64_t)(i + 1)) >> 64);
        const int32_t t = out[i];
        out[i] = out[j];
        out[j] = t;
    }
}

struct TrainStepArgs {
    TrainNet n;
    const float* din;                            // [rows][dims[0]]
    const float* dout;                           // [rows][dims[L]]
    const int* idx;                              // [B] dataset rows of this batch; null: rows row0 .. row0 + B - 1
    long long idx_stride;                        // ints from member e's idx to member e + 1's
    int row0;
    int B;
    float* part;                                 // [E][tiles][n_params]
    float* lossp;                                // [E][tiles] sum of squared errors
    const TrainMon* stop;                        // member e's state at [2 e] (the parity is in the pointer); null: none
    TrainHead h;                                 // read by the NLL instantiation only
};

struct TrainMseArgs {
    TrainNet n;
    const float* din;
    const float* dout;
    int B;                                       // rows per batch; tile blockIdx.x = (batch, tile of the batch)
    int tiles_per_batch;
    float* tile_loss;                            // [E][batches * tiles_per_batch] or null
    float* colsq;                                // [E][batches * tiles_per_batch][O] or null
    const TrainMon* stop;                        // as TrainStepArgs::stop
    TrainHead h;                                 // read by the NLL instantiation only
};

struct TrainUpdateArgs {
    TrainNet n;
    float* theta;                                // [E][n_params], as m, v
    float* m;
    float* v;
    const float* part;                           // [E][ntiles][n_params]
    const float* lossp;                          // [E][ntiles]
    int ntiles;
    int rule;
    float lr, b1, b2, omb1, omb2, rho, omrho, eps;
    double lr_d, b1_d, b2_d;
    double* pows;                                // [E][2][2]: (b1^t, b2^t) read at [parity], written at [parity ^ 1]
    int parity;
    float inv_count;                             // 1 / (B O)
    float gscale;                                // 2 / (B O): the MSE gradient's factor, applied to the summed shares
    float* loss_acc;                             // += the batch loss (TR_RULE_NONE: = )
    int loss_stride;                             // floats from member e's loss_acc to member e + 1's
    float* grads_out;                            // TR_RULE_NONE: the summed gradient [E][n_params]
    float wd[TR_MAX_LAYERS];                     // lambda_l of W_l; all zero: no decay
    float lrwd[TR_MAX_LAYERS];                   // float32 lr * lambda_l (TR_DECAY_DECOUPLED)
    int wd_mode;                                 // TR_DECAY_*
    int wd_on;                                   // is any lambda_l != 0?
    const TrainMon* stop;                        // as TrainStepArgs::stop
    TrainHead h;                                 // read by the NLL instantiation only
};

#ifdef BBMPC_TU_TRAIN

// has member e stopped?  (uniform over the workgroup: one scalar load)
__device__ __forceinline__ bool tr_stopped(const TrainMon* stop, int e) { return stop && stop[2 * e].stopped != 0; }

// The layer parameter i of theta belongs to; returns whether it is a bias.
__device__ __forceinline__ bool tr_param_layer(const TrainNet& n, int i, int& l) {
    const bool bias = i >= n.boff[0];
    l = n.L - 1;
    if (bias) {
        while (i < n.boff[l]) --l;
    } else {
        while (i < n.woff[l]) --l;
    }
    return bias;
}

// Parameter i (layer l) = w in every layout the step kernel reads; mo: the member's offset into the operand packs.
__device__ __forceinline__ void tr_write_layouts(const TrainNet& n, size_t mo, int i, int l, bool bias, float w) {
    if (bias) {
        n.bp[l][mo + i - n.boff[l]] = w;
    } else {
        const int out = n.dims[l + 1];
        const int k = i - n.woff[l];
        const int fi = k / out, fo = k - fi * out;
        n.wf[l][mo + train_wf_index(n.tiles[l], fi, fo)] = w;
        n.wr[l][mo + train_wr_index(n.tiles[l + 1], fi, fo)] = w;
    }
}

// tr_param_layer with the head: its parameters lie behind b_{L-1} and count as layer L - 1 (the decay W_v sees).
template <bool NLL>
__device__ __forceinline__ bool tr_locate(const TrainNet& n, const TrainHead& h, int i, int& l, bool& head) {
    head = NLL && i >= h.woff;
    if (head) {
        l = n.L - 1;
        return i >= h.boff;
    }
    return tr_param_layer(n, i, l);
}

// tr_write_layouts with the head: W_v is packed like W_{L-1} (same tile counts), b_v like b_{L-1}.
template <bool NLL>
__device__ __forceinline__ void tr_store_layouts(const TrainNet& n, const TrainHead& h, size_t mo, int i, int l, bool bias, bool head, float w) {
    if (NLL && head) {
        if (bias) {
            h.bp[mo + i - h.boff] = w;
        } else {
            const int out = n.dims[n.L];
            const int k = i - h.woff;
            const int fi = k / out, fo = k - fi * out;
            h.wf[mo + train_wf_index(n.tiles[n.L - 1], fi, fo)] = w;
            h.wr[mo + train_wr_index(n.tiles[n.L], fi, fo)] = w;
        }
    } else {
        tr_write_layouts(n, mo, i, l, bias, w);
    }
}

// softplus and the logistic function in their accurate forms (expf / log1pf): DenseTrainer._softplus's max(x, 0) +
// log1p(e^-|x|), and e^-|x| on either side of 0 so that neither tail cancels.
__device__ __forceinline__ float tr_softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float tr_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    const float d = 1.0f + e;
    return x >= 0.0f ? 1.0f / d : e / d;
}

// The soft clamp of the head's output z between lo = min_lv and hi = max_lv: lv, and dlv / dz.
__device__ __forceinline__ void tr_logvar(float z, float lo, float hi, float& lv, float& dlv) {
    const float a = hi - z;
    const float lv1 = hi - tr_softplus(a);
    const float b = lv1 - lo;
    lv = lo + tr_softplus(b);
    dlv = tr_sigmoid(b) * tr_sigmoid(a);
}

__device__ __forceinline__ int tr_addr(int f, int p) {                   // feature f of row p in a tile array
    return (((f >> 4) * 64) + (((f & 15) >> 2) * 16 + p)) * 4 + (f & 3);
}

// d act / dx from the layer's output y (z: the pre-activation, read only where train_needs_pre): DenseTrainer._act_grad's
// forms.  relu / elu / selu / leaky_relu test y > 0, which is x > 0; the three below cannot be asked through act_grad
// without x.
__device__ __forceinline__ float train_act_grad(float y, float z, int act) {
    switch (act) {
    case ACT_SOFTPLUS: return 1.0f - __builtin_amdgcn_exp2f(-BB_LOG2E * y);           // sigma(x) = 1 - e^-y
    case ACT_HARD_SIGMOID: return (y > 0.0f && y < 1.0f) ? 0.2f : 0.0f;
    case ACT_RELU6: return (y > 0.0f && y < 6.0f) ? 1.0f : 0.0f;
    case ACT_SWISH: return act_grad(z, y, act);
    default: return act_grad(y, y, act);
    }
}

// acc += M[ot] . in over IT k tiles; W points at the pack's (ot, 0, lane)
__device__ __forceinline__ tr_f32x4 tr_tile_product(const tr_f32x4* __restrict__ W, int in_off, int IT, int lane, tr_f32x4 acc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
#pragma unroll 4
    for (int it = 0; it < IT; ++it) {
        const tr_f32x4 b = *reinterpret_cast<const tr_f32x4*>(smem + in_off + (it * 64 + lane) * 4);
        const tr_f32x4 a = W[(size_t)it * 64];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
    }
    return acc;
}

// The tile's dataset rows (scratch words 0 .. 15, -1 past the batch) and its input tile y_0.  Ends with a barrier.
__device__ __forceinline__ void tr_load_input(const TrainNet& n, const float* din, const int* idx, int row0, int n0, int valid,
                                              int tid, int nthr) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    int* rows = reinterpret_cast<int*>(smem + n.soff);
    const int D = n.dims[0];
    if (tid < TR_ROWS) rows[tid] = tid < valid ? (idx ? idx[n0 + tid] : row0 + n0 + tid) : -1;
    for (int i = tid; i < n.tiles[0] * 256; i += nthr) smem[n.yoff[0] + i] = 0.0f;
    __syncthreads();
    for (int i = tid; i < TR_ROWS * D; i += nthr) {
        const int pp = i / D, f = i - pp * D;
        const int r = rows[pp];
        if (r >= 0) smem[n.yoff[0] + tr_addr(f, pp)] = din[(size_t)r * D + f];
    }
    __syncthreads();
}

// The forward stack: y_{l+1} = act(y_l W_l + b_l) for every layer, all resident; mo: the member's offset into the operand
// packs.  NLL: in the last layer the head's z = y_{L-1} W_v + b_v is formed next to the mean's tile, into h.zoff.  Ends with a
// barrier.
template <bool NLL>
__device__ __forceinline__ void tr_forward(const TrainNet& n, const TrainHead& h, size_t mo, int wave, int lane) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    for (int l = 0; l < n.L; ++l) {
        const int IT = n.tiles[l], OT = n.tiles[l + 1], a = n.act[l];
        const tr_f32x4* __restrict__ W = reinterpret_cast<const tr_f32x4*>(n.wf[l] + mo);
        for (int ot = wave; ot < OT; ot += n.nw) {
            tr_f32x4 acc = *reinterpret_cast<const tr_f32x4*>(n.bp[l] + mo + ot * 16 + (lane >> 4) * 4);     // the bias enters as C
            acc = tr_tile_product(W + (size_t)ot * IT * 64 + lane, n.yoff[l], IT, lane, acc);
            if (n.zoff[l] >= 0) *reinterpret_cast<tr_f32x4*>(smem + n.zoff[l] + (ot * 64 + lane) * 4) = acc;
            acc.x = apply_act(acc.x, a); acc.y = apply_act(acc.y, a); acc.z = apply_act(acc.z, a); acc.w = apply_act(acc.w, a);
            *reinterpret_cast<tr_f32x4*>(smem + n.yoff[l + 1] + (ot * 64 + lane) * 4) = acc;
            if (NLL && l == n.L - 1) {
                tr_f32x4 zv = *reinterpret_cast<const tr_f32x4*>(h.bp + mo + ot * 16 + (lane >> 4) * 4);
                zv = tr_tile_product(reinterpret_cast<const tr_f32x4*>(h.wf + mo) + (size_t)ot * IT * 64 + lane, n.yoff[l], IT, lane, zv);
                *reinterpret_cast<tr_f32x4*>(smem + h.zoff + (ot * 64 + lane) * 4) = zv;
            }
        }
        __syncthreads();
    }
}

// MON: is the launch part of a monitored fit (q.stop set)?  The unmonitored instantiation carries no test of it.
// NLL: does the network carry a log-variance head (q.h set; the loss is the Gaussian NLL)?  Likewise.
template <bool MON, bool NLL>
__global__ __launch_bounds__(1024) void k_train_fwd_bwd(TrainStepArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (MON && tr_stopped(q.stop, blockIdx.y)) return;
    const TrainNet& n = q.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = n.nw, nthr = nw * 64;
    const int n0 = blockIdx.x * TR_ROWS;
    const int valid = q.B - n0 < TR_ROWS ? q.B - n0 : TR_ROWS;
    const int L = n.L, O = n.dims[L];
    const int p = lane & 15, g = lane >> 4;
    const int* rows = reinterpret_cast<const int*>(smem + n.soff);
    float* words = smem + n.soff + 64;                              // one word per thread
    const int e = blockIdx.y;                                       // the member: uniform, so what follows is scalar arithmetic
    const size_t mo = (size_t)e * n.pstride;
    const size_t slot = (size_t)e * gridDim.x + blockIdx.x;         // (member, tile)
    float* part = q.part + slot * n.n_params;

    tr_load_input(n, q.din, q.idx ? q.idx + e * q.idx_stride : nullptr, q.row0, n0, valid, tid, nthr);
    tr_forward<NLL>(n, q.h, mo, wave, lane);

    if (NLL) {
        // ---- delta_mu = act'(y_L) (diff inv) in place of y_L, delta_z = 0.5 (1 - wsq) dlv/dz in place of z; each thread's
        // wsq + lv go to its word.  The exact 0.5 leaves k_train_update its single 2 / (B O) for every summed gradient.
        const int a = n.act[L - 1];
        const int r = rows[p];
        float sq = 0.0f;
        for (int t = wave; t < n.tiles[L]; t += nw) {
            float* yp = smem + n.yoff[L] + (t * 64 + lane) * 4;
            float* zp = smem + q.h.zoff + (t * 64 + lane) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int f = 16 * t + 4 * g + c;
                float d = 0.0f, dz = 0.0f;
                if (r >= 0 && f < O) {
                    const float y = yp[c];
                    const float z = n.zoff[L - 1] >= 0 ? smem[n.zoff[L - 1] + (t * 64 + lane) * 4 + c] : y;
                    const float diff = y - q.dout[(size_t)r * O + f];
                    float lv, dlv;
                    tr_logvar(zp[c], q.h.min_lv[f], q.h.max_lv[f], lv, dlv);
                    const float inv = expf(-lv);
                    const float wsq = diff * diff * inv;
                    sq = sq + (wsq + lv);
                    d = train_act_grad(y, z, a) * (diff * inv);
                    dz = 0.5f * (1.0f - wsq) * dlv;
                }
                yp[c] = d;
                zp[c] = dz;
            }
        }
        words[tid] = sq;
    } else {
        // ---- delta_{L-1} = act'(y_L) * (y_L - t), in place (2 / (B O): k_train_update); each thread's squared errors go to its word
        const int a = n.act[L - 1];
        const int r = rows[p];
        float sq = 0.0f;
        for (int t = wave; t < n.tiles[L]; t += nw) {
            float* yp = smem + n.yoff[L] + (t * 64 + lane) * 4;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int f = 16 * t + 4 * g + c;
                float d = 0.0f;
                if (r >= 0 && f < O) {
                    const float y = yp[c];
                    const float z = n.zoff[L - 1] >= 0 ? smem[n.zoff[L - 1] + (t * 64 + lane) * 4 + c] : y;
                    const float diff = y - q.dout[(size_t)r * O + f];
                    sq = sq + diff * diff;
                    d = train_act_grad(y, z, a) * diff;
                }
                yp[c] = d;
            }
        }
        words[tid] = sq;
    }
    __syncthreads();
    // ---- the tile's sum of squared errors: wave 0, waves ascending per lane, then lane groups, then rows
    if (wave == 0) {
        float s = 0.0f;
        for (int w = 0; w < nw; ++w) s = s + words[w * 64 + lane];
        const float s0 = __shfl(s, p), s1 = __shfl(s, 16 + p), s2 = __shfl(s, 32 + p), s3 = __shfl(s, 48 + p);
        const float rs = ((s0 + s1) + s2) + s3;
        float tot = 0.0f;
        for (int j = 0; j < TR_ROWS; ++j) tot = tot + __shfl(rs, j);
        if (lane == 0) q.lossp[slot] = tot;
    }

    // ---- backward sweep: delta_l sits in y_{l+1}'s tiles
    for (int l = L - 1; l >= 0; --l) {
        const int IT = n.tiles[l], OT = n.tiles[l + 1], in = n.dims[l], out = n.dims[l + 1];
        // dW_l = y_l^T delta_l: K = the 16 rows, row r = 4 s + g in product s
        for (int pr = wave; pr < IT * OT; pr += nw) {
            const int it = pr / OT, ot = pr - it * OT;
            const float* xa = smem + n.yoff[l] + (it * 64 + (p >> 2) * 16) * 4 + (p & 3);
            const float* db = smem + n.yoff[l + 1] + (ot * 64 + (p >> 2) * 16) * 4 + (p & 3);
            tr_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[(4 * s + g) * 4], db[(4 * s + g) * 4], acc, 0, 0, 0);
            const int fo = 16 * ot + p;
            if (fo < out) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int fi = 16 * it + 4 * g + c;
                    if (fi < in) part[n.woff[l] + (size_t)fi * out + fo] = acc[c];
                }
            }
        }
        // db_l = column sums of delta_l in row order
        for (int o = tid; o < out; o += nthr) {
            const float* dp = smem + n.yoff[l + 1] + tr_addr(o, 0);
            float s = 0.0f;
#pragma unroll
            for (int r = 0; r < TR_ROWS; ++r) s = s + dp[r * 4];
            part[n.boff[l] + o] = s;
        }
        if (NLL && l == L - 1) {
            // dW_v = y_{L-1}^T delta_z and db_v: the two loops above on the head's tiles
            for (int pr = wave; pr < IT * OT; pr += nw) {
                const int it = pr / OT, ot = pr - it * OT;
                const float* xa = smem + n.yoff[l] + (it * 64 + (p >> 2) * 16) * 4 + (p & 3);
                const float* db = smem + q.h.zoff + (ot * 64 + (p >> 2) * 16) * 4 + (p & 3);
                tr_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[(4 * s + g) * 4], db[(4 * s + g) * 4], acc, 0, 0, 0);
                const int fo = 16 * ot + p;
                if (fo < out) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const int fi = 16 * it + 4 * g + c;
                        if (fi < in) part[q.h.woff + (size_t)fi * out + fo] = acc[c];
                    }
                }
            }
            for (int o = tid; o < out; o += nthr) {
                const float* dp = smem + q.h.zoff + tr_addr(o, 0);
                float s = 0.0f;
#pragma unroll
                for (int r = 0; r < TR_ROWS; ++r) s = s + dp[r * 4];
                part[q.h.boff + o] = s;
            }
        }
        if (l == 0) break;
        // g = delta_l W_l^T; NLL, at the last layer: + delta_z W_v^T on the same accumulator, the mean's k tiles first
        {
            const tr_f32x4* __restrict__ W = reinterpret_cast<const tr_f32x4*>(n.wr[l] + mo);
            for (int ot = wave; ot < IT; ot += nw) {
                tr_f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                acc = tr_tile_product(W + (size_t)ot * OT * 64 + lane, n.yoff[l + 1], OT, lane, acc);
                if (NLL && l == L - 1)
                    acc = tr_tile_product(reinterpret_cast<const tr_f32x4*>(q.h.wr + mo) + (size_t)ot * OT * 64 + lane, q.h.zoff, OT, lane, acc);
                *reinterpret_cast<tr_f32x4*>(smem + n.goff + (ot * 64 + lane) * 4) = acc;
            }
        }
        __syncthreads();
        // delta_{l-1} = act'(y_l) * g, in place of y_l; zero past the batch and past the layer's width
        {
            const int a = n.act[l - 1];
            const bool live = rows[p] >= 0;
            for (int t = wave; t < IT; t += nw) {
                float* yp = smem + n.yoff[l] + (t * 64 + lane) * 4;
                const float* gp = smem + n.goff + (t * 64 + lane) * 4;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int f = 16 * t + 4 * g + c;
                    float d = 0.0f;
                    if (live && f < in) {
                        const float y = yp[c];
                        const float z = n.zoff[l - 1] >= 0 ? smem[n.zoff[l - 1] + (t * 64 + lane) * 4 + c] : y;
                        d = train_act_grad(y, z, a) * gp[c];
                    }
                    yp[c] = d;
                }
            }
        }
        __syncthreads();
    }
}

// Forward only on rows b * B + 16 t .. of batch b (tile t of the batch): squared errors per output column, and their sum.
// Grid (batches * tiles_per_batch, E): every member on the same rows.  NLL: per output column the sum of wsq + lv instead.
template <bool MON, bool NLL>
__global__ __launch_bounds__(1024) void k_train_forward_mse(TrainMseArgs q) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    if (MON && tr_stopped(q.stop, blockIdx.y)) return;
    const TrainNet& n = q.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nthr = n.nw * 64;
    const int batch = blockIdx.x / q.tiles_per_batch, tile = blockIdx.x - batch * q.tiles_per_batch;
    const int n0 = tile * TR_ROWS;
    const int valid = q.B - n0 < TR_ROWS ? q.B - n0 : TR_ROWS;
    const int L = n.L, O = n.dims[L];
    const int* rows = reinterpret_cast<const int*>(smem + n.soff);
    float* words = smem + n.soff + 64;
    const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;          // (member, tile)
    tr_load_input(n, q.din, nullptr, batch * q.B, n0, valid, tid, nthr);
    tr_forward<NLL>(n, q.h, (size_t)blockIdx.y * n.pstride, wave, lane);
    for (int o = tid; o < 1024; o += nthr) {
        float s = 0.0f;
        if (NLL) {
            if (o < O) {
                const float lo = q.h.min_lv[o], hi = q.h.max_lv[o];
                for (int r = 0; r < valid; ++r) {
                    const float d = smem[n.yoff[L] + tr_addr(o, r)] - q.dout[(size_t)rows[r] * O + o];
                    float lv, dlv;
                    tr_logvar(smem[q.h.zoff + tr_addr(o, r)], lo, hi, lv, dlv);
                    s = s + (d * d * expf(-lv) + lv);
                }
            }
        } else if (o < O)
            for (int r = 0; r < valid; ++r) {
                const float d = smem[n.yoff[L] + tr_addr(o, r)] - q.dout[(size_t)rows[r] * O + o];
                s = s + d * d;
            }
        words[o] = s;
        if (q.colsq && o < O) q.colsq[slot * O + o] = s;
    }
    __syncthreads();
    if (wave == 0 && q.tile_loss) {
        float s = 0.0f;
        for (int o = lane; o < O; o += 64) s = s + words[o];
        float tot = 0.0f;
        for (int j = 0; j < 64; ++j) tot = tot + __shfl(s, j);
        if (lane == 0) q.tile_loss[slot] = tot;
    }
}

// val_out[0] = mean over the batches of (sum of the batch's tile losses in tile order) / (B O); NaN without a batch.
// Grid (1, E): member e reads tile_loss[e][..], uses batch_mse[e][batches] and writes val_out[e * val_stride].
__global__ void k_train_val_reduce(const float* tile_loss, int batches, int tiles_per_batch, float inv_count, float* batch_mse, float* val_out,
                                   int val_stride, const TrainMon* stop) {
    const int e = blockIdx.y;
    if (tr_stopped(stop, e)) return;
    tile_loss += (size_t)e * batches * tiles_per_batch;
    batch_mse += (size_t)e * batches;
    val_out += (size_t)e * val_stride;
    for (int b = threadIdx.x; b < batches; b += blockDim.x) {
        float s = 0.0f;
        for (int t = 0; t < tiles_per_batch; ++t) s = s + tile_loss[(size_t)b * tiles_per_batch + t];
        batch_mse[b] = s * inv_count;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int b = 0; b < batches; ++b) s = s + batch_mse[b];
        val_out[0] = s / (float)batches;
    }
}

// rms_out[e][o] = sqrt(sum over tiles (ascending) of colsq[e][tile][o] / rows); grid (ceil(O / 64), E)
__global__ void k_train_rms_reduce(const float* colsq, int tiles, int O, float inv_rows, float* rms_out) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= O) return;
    colsq += (size_t)blockIdx.y * tiles * O;
    rms_out += (size_t)blockIdx.y * O;
    float s = 0.0f;
    for (int t = 0; t < tiles; ++t) s = s + colsq[(size_t)t * O + o];
    rms_out[o] = sqrtf(s * inv_rows);
}

// Grid (ceil(n_params / 256), E).  REG: does the launch decay a kernel or belong to a monitored fit?  The instantiation
// without either is the update as it has always been, instruction for instruction: an early test of q.stop in front of the
// other arguments' loads cost a default fit 0.5 % when it was there (profiles/train_hip.md).
// NLL: does theta end with a log-variance head (q.h set)?  W_v then decays with the last layer's lambda, b_v never.
template <bool REG, bool NLL>
__global__ __launch_bounds__(256) void k_train_update(TrainUpdateArgs q) {
    const TrainNet& n = q.n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = blockIdx.y;                                       // the member: every offset below is scalar
    const size_t po = (size_t)e * n.n_params, mo = (size_t)e * n.pstride;
    const float* lossp = q.lossp + (size_t)e * q.ntiles;
    const float* part = q.part + po * q.ntiles;
    double* pows = q.pows + e * 4;
    float* loss_acc = q.loss_acc + (size_t)e * q.loss_stride;
    float* theta = q.theta + po;
    float* mm = q.m + po;
    float* vv = q.v + po;
    if (REG && tr_stopped(q.stop, e)) {                            // the powers keep their value and move to the parity the next step reads
        if (q.rule == TR_RULE_ADAM && i == 0) {
            pows[(q.parity ^ 1) * 2 + 0] = pows[q.parity * 2 + 0];
            pows[(q.parity ^ 1) * 2 + 1] = pows[q.parity * 2 + 1];
        }
        return;
    }
    if (i == 0) {
        float s = 0.0f;
        for (int t = 0; t < q.ntiles; ++t) s = s + lossp[t];
        const float loss = s * q.inv_count;
        if (q.rule == TR_RULE_NONE) loss_acc[0] = loss;
        else loss_acc[0] = loss_acc[0] + loss;
    }
    double b1t = 1.0, b2t = 1.0;
    if (q.rule == TR_RULE_ADAM) {
        b1t = pows[q.parity * 2 + 0] * q.b1_d;
        b2t = pows[q.parity * 2 + 1] * q.b2_d;
        if (i == 0) {
            pows[(q.parity ^ 1) * 2 + 0] = b1t;
            pows[(q.parity ^ 1) * 2 + 1] = b2t;
        }
    }
    if (i >= n.n_params) return;
    float gsum = 0.0f;
    for (int t = 0; t < q.ntiles; ++t) gsum = gsum + part[(size_t)t * n.n_params + i];
    gsum = gsum * q.gscale;
    if (q.rule == TR_RULE_NONE) {
        q.grads_out[po + i] = gsum;
        return;
    }
    // The parameter's layer is looked up before the rule where a decay needs it (wd_on, uniform) and behind the store of the
    // parameter otherwise, where it has always been.
    const bool decay = REG && q.wd_on;
    int l = 0;
    bool bias = false, head = false;
    float lam = 0.0f;
    if (decay) {
        bias = tr_locate<NLL>(n, q.h, i, l, head);
        lam = bias ? 0.0f : q.wd[l];
    }
    const float w0 = theta[i];
    float w = w0;
    if (lam != 0.0f && q.wd_mode == TR_DECAY_L2) gsum = __fmaf_rn(lam, w0, gsum);
    if (q.rule == TR_RULE_SGD) {
        w = w + (-q.lr) * gsum;
    } else if (q.rule == TR_RULE_RMSPROP) {
        const float v = q.rho * vv[i] + q.omrho * (gsum * gsum);
        vv[i] = v;
        w = w + (-q.lr) * (gsum / (sqrtf(v) + q.eps));
    } else {
        const float lr_t = (float)(q.lr_d * sqrt(1.0 - b2t) / (1.0 - b1t));
        const float m = q.b1 * mm[i] + q.omb1 * gsum;
        const float v = q.b2 * vv[i] + q.omb2 * (gsum * gsum);
        mm[i] = m;
        vv[i] = v;
        w = w + (-lr_t) * (m / (sqrtf(v) + q.eps));
    }
    if (lam != 0.0f && q.wd_mode == TR_DECAY_DECOUPLED) w = __fmaf_rn(-q.lrwd[l], w0, w);
    theta[i] = w;
    if (!decay) bias = tr_locate<NLL>(n, q.h, i, l, head);
    tr_store_layouts<NLL>(n, q.h, mo, i, l, bias, head, w);         // every layout the step kernel reads
}

// Epoch k's decision for every member, behind k_train_val_reduce.  Grid (ceil(n_params / 256), E), or (1, E) with
// best_theta null (nothing to restore later: no snapshot).  val: the epoch's validation loss of member 0, member e's
// val_stride floats further.  v improves on best if v < best - min_delta in float32: NaN never does, and the first finite
// (or -inf) v does, whatever min_delta is.
__global__ __launch_bounds__(256) void k_train_monitor(TrainMon* mon, const float* val, int val_stride, int k, int patience, float min_delta,
                                                       const float* theta, float* best_theta, int n_params) {
    const int e = blockIdx.y;
    const TrainMon s = mon[2 * e + (k & 1)];
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (s.stopped) {
        if (first) mon[2 * e + ((k & 1) ^ 1)] = s;
        return;
    }
    const float v = val[(size_t)e * val_stride];
    const bool better = v < s.best - min_delta;
    if (first) {
        TrainMon o = s;
        if (better) {
            o.best = v;
            o.best_epoch = k;
            o.wait = 0;
        } else {
            o.wait = s.wait + 1;
        }
        if (patience > 0 && o.wait >= patience) o.stopped = k + 1;
        mon[2 * e + ((k & 1) ^ 1)] = o;
    }
    if (better && best_theta) {
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n_params) best_theta[(size_t)e * n_params + i] = theta[(size_t)e * n_params + i];
    }
}

// best_theta -> theta and every layout, for the members with a best epoch; mon: the state after the last epoch.
// Grid (ceil(n_params / 256), E).  NLL: the head's parameters and its three layouts too (h).
template <bool NLL>
__global__ __launch_bounds__(256) void k_train_restore(TrainNet n, const TrainMon* mon, const float* best_theta, float* theta, TrainHead h) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int e = blockIdx.y;
    if (mon[2 * e].best_epoch < 0 || i >= n.n_params) return;
    const float w = best_theta[(size_t)e * n.n_params + i];
    theta[(size_t)e * n.n_params + i] = w;
    int l;
    bool head;
    const bool bias = tr_locate<NLL>(n, h, i, l, head);
    tr_store_layouts<NLL>(n, h, (size_t)e * n.pstride, i, l, bias, head, w);
}

#endif  // BBMPC_TU_TRAIN

}  // namespace bbmpc
