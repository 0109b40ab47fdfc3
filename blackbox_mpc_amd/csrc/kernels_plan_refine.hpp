// Plan refinement on the device (bbmpc_refine_plans, bbmpc_set_grad_refine): the projected ascent step,
// the keep-best and the move of CEM's candidate columns into rows and back, around k_plan_grad (kernels_plan_grad.hpp).
//
// k_refine_step.  One element x[b, t, u] per lane (four when the row length allows float4), in plain float32, no contraction
// into fused multiply-adds, in this order -- tests/plan_refine_util.py states the same order in NumPy:
//     Adam:  m = 0.9f * m + 0.1f * g
//            v = 0.999f * v + (0.001f * g) * g
//            step = (m / c1) / (sqrtf(v / c2) + 1e-8f)        c1 = 1 - 0.9^k, c2 = 1 - 0.999^k, k the 1-based step number
//     SGD:   step = g
//     step = isfinite(step) ? step : 0
//     x = min(max(x + lr * step, lo[u]), hi[u])
// c1 and c2 arrive as arguments: the host forms 0.9^k and 0.999^k by k float32 multiplications (refine_bias_correction below),
// so that the kernel has no pow and the restatement can repeat the same products.
//
// k_refine_keep_best.  One workgroup per row: returns[b] scored x[b]; the row and its return replace the stored best when
// returns[b] > best_ret[b] (false for a NaN return), or unconditionally on the first call of a refinement.
//
// k_refine_gather / k_refine_scatter.  Columns [N - M, N) of the sample buffer [A][HU][Nst] (particle-minor) <-> rows
// [A * M][HU], row a * M + c = column N - M + c of agent a; the gather also repeats agent a's state over its M rows.  The
// column index is the fastest over lanes, so the buffer side is contiguous.  Columns n >= N and n < N - M are never touched.
//
// No atomics, nothing depends on the grid: an element's arithmetic is the same wherever it runs.
#pragma once
#include <hip/hip_runtime.h>

namespace bbmpc {

constexpr int REFINE_THREADS = 256;
constexpr int REFINE_ADAM = 0, REFINE_SGD = 1;
constexpr int REFINE_MAX_STEPS = 64;

struct RefineStepArgs {
    float* x;                  // [n] the plans, updated in place
    const float* g;            // [n] dR/dx of k_plan_grad
    float* m;                  // [n] Adam's first moment  (not read by SGD)
    float* v;                  // [n] Adam's second moment
    const float* lo;           // [U]
    const float* hi;           // [U]
    long n;                    // B * Hq * U
    int U;
    int method;
    float lr, c1, c2;
};

// (1 - 0.9^k, 1 - 0.999^k) by k float32 products each
inline void refine_bias_correction(int k, float& c1, float& c2) {
    float p1 = 1.0f, p2 = 1.0f;
    for (int i = 0; i < k; ++i) {
        p1 = p1 * 0.9f;
        p2 = p2 * 0.999f;
    }
    c1 = 1.0f - p1;
    c2 = 1.0f - p2;
}

#ifdef BBMPC_TU_MLP

__device__ __forceinline__ float refine_update(float x, float g, float& m, float& v, float lo, float hi, int method, float lr, float c1, float c2) {
    float step = g;                                                  // (the unit is built with -ffp-contract=off)
    if (method == REFINE_ADAM) {
        const float a = 0.9f * m, b = 0.1f * g;
        m = a + b;
        const float c = 0.999f * v, d = (0.001f * g) * g;
        v = c + d;
        const float mh = m / c1, vh = v / c2;
        step = mh / (sqrtf(vh) + 1e-8f);
    }
    if (!isfinite(step)) step = 0.0f;
    const float moved = lr * step;
    return fminf(fmaxf(x + moved, lo), hi);
}

template <bool V4>
__global__ void k_refine_step(RefineStepArgs q) {
    const long i = (long)blockIdx.x * REFINE_THREADS + threadIdx.x;
    if constexpr (V4) {
        const long e0 = i * 4;
        if (e0 >= q.n) return;                                       // (n is a multiple of 4 in this form)
        float4 x = reinterpret_cast<const float4*>(q.x)[i];
        const float4 g = reinterpret_cast<const float4*>(q.g)[i];
        float4 m = make_float4(0.f, 0.f, 0.f, 0.f), v = m;
        if (q.method == REFINE_ADAM) {
            m = reinterpret_cast<const float4*>(q.m)[i];
            v = reinterpret_cast<const float4*>(q.v)[i];
        }
        const int U = q.U;
        const int u0 = (int)(e0 % U), u1 = (int)((e0 + 1) % U), u2 = (int)((e0 + 2) % U), u3 = (int)((e0 + 3) % U);
        x.x = refine_update(x.x, g.x, m.x, v.x, q.lo[u0], q.hi[u0], q.method, q.lr, q.c1, q.c2);
        x.y = refine_update(x.y, g.y, m.y, v.y, q.lo[u1], q.hi[u1], q.method, q.lr, q.c1, q.c2);
        x.z = refine_update(x.z, g.z, m.z, v.z, q.lo[u2], q.hi[u2], q.method, q.lr, q.c1, q.c2);
        x.w = refine_update(x.w, g.w, m.w, v.w, q.lo[u3], q.hi[u3], q.method, q.lr, q.c1, q.c2);
        reinterpret_cast<float4*>(q.x)[i] = x;
        if (q.method == REFINE_ADAM) {
            reinterpret_cast<float4*>(q.m)[i] = m;
            reinterpret_cast<float4*>(q.v)[i] = v;
        }
    } else {
        if (i >= q.n) return;
        const int u = (int)(i % q.U);
        float m = 0.0f, v = 0.0f;
        if (q.method == REFINE_ADAM) { m = q.m[i]; v = q.v[i]; }
        q.x[i] = refine_update(q.x[i], q.g[i], m, v, q.lo[u], q.hi[u], q.method, q.lr, q.c1, q.c2);
        if (q.method == REFINE_ADAM) { q.m[i] = m; q.v[i] = v; }
    }
}

// grid (B), block (64): row b of x [B][row] into best [B][row] when its return is the best so far
__global__ void k_refine_keep_best(const float* __restrict__ x, const float* __restrict__ returns, float* __restrict__ best,
                                   float* __restrict__ best_ret, int row, int first) {
    const int b = blockIdx.x;
    const float r = returns[b];
    const bool take = first || r > best_ret[b];                      // (NaN > anything is false)
    __syncthreads();                                                 // every lane has read best_ret[b] before lane 0 replaces it
    if (!take) return;
    const size_t o = (size_t)b * row;
    for (int j = threadIdx.x; j < row; j += blockDim.x) best[o + j] = x[o + j];
    if (threadIdx.x == 0) best_ret[b] = r;
}

// grid (ceil((HU * M + S * M) / REFINE_THREADS), A).  Work item w < HU * M: element j = w / M of column c = w % M;
// the rest: state element s of row c.
__global__ void k_refine_gather(const float* __restrict__ samples, const float* __restrict__ state, float* __restrict__ rows,
                                float* __restrict__ row_states, int HU, int S, int Nst, int N, int M) {
    const int a = blockIdx.y;
    const int w = blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (w < HU * M) {
        const int j = w / M, c = w - j * M;
        rows[((size_t)a * M + c) * HU + j] = samples[((size_t)a * HU + j) * Nst + (N - M + c)];
    } else if (w < HU * M + S * M) {
        const int e = w - HU * M, s = e / M, c = e - s * M;
        row_states[((size_t)a * M + c) * S + s] = state[(size_t)a * S + s];
    }
}

// grid (ceil(HU * M / REFINE_THREADS), A): the rows back over columns [N - M, N)
__global__ void k_refine_scatter(const float* __restrict__ rows, float* __restrict__ samples, int HU, int Nst, int N, int M) {
    const int a = blockIdx.y;
    const int w = blockIdx.x * REFINE_THREADS + threadIdx.x;
    if (w >= HU * M) return;
    const int j = w / M, c = w - j * M;
    samples[((size_t)a * HU + j) * Nst + (N - M + c)] = rows[((size_t)a * M + c) * HU + j];
}

#endif  // BBMPC_TU_MLP

}  // namespace bbmpc
