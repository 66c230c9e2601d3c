// Multi-tensor AdamW step: ONE launch updates every parameter tensor of the model (the reference builds
// ~530 parameter groups, one per tensor: train_tasks.py:400-420, train_concap.py:420-440).
// Arithmetic = pytorch-transformers 1.0.0 `AdamW.step` (requirements.txt:1; the package is not vendored in
// the reference tree - restated in oracle/adamw_oracle.py):
//   m = beta1 m + (1 - beta1) g;  v = beta2 v + (1 - beta2) g^2;  p -= step_size * m / (sqrt(v) + eps)
//   then decoupled weight decay on the UPDATED value:  p -= lr * wd * p
// with step_size = lr * sqrt(1 - beta2^t) / (1 - beta1^t) when correct_bias else lr (computed on the host).
// HBM-bound: 16 B read + 12 B written per parameter; blocks walk fixed-size chunks listed in a table.
//
// Global-norm clipping, a gradient scale and the skip of a non-finite step ride on the same tables (vilbert_hip_ext.h):
//   grad_sumsq_kernel        one block per chunk -> one fp32 partial sum of squares per chunk (4 B read per parameter)
//   grad_norm_finish_kernel  one block: partials -> {sum of squares, norm, coef, finite flag, skipped steps} on the device
//   adamw_kernel             given that state, the update with every gradient multiplied by coef on load; no store at all when
//                            the step is skipped
// No atomics and a fixed summation order everywhere: the same gradients give the same bits. The coefficient never visits the
// host, so the three launches are graph-capturable. The gradients themselves are only read.
//
// Multi-tensor RAdam step (vilbert_hip_optim.h; the reference's vilbert/optimization.py:55-98, `--optim RAdam` of train_tasks.py):
//   radam_kernel             the per-tensor hyper-parameters - step size, rectified flag, lr * wd - come from a table of their
//                            own the host computes in double
//
// Every kernel but grad_norm_finish_kernel is the chunk walk of optim_walk.h around its element function: one block per chunk,
// 16-byte accesses where the tensor's base pointers allow them, the optional state of the norm pass read once per block.
#include <cmath>

#include "optim_walk.h"
#include "../../include/vilbert_hip_optim.h"

namespace {

using namespace optim_walk;

__device__ __forceinline__ void adamw_element(const vb_adamw_tensor& t, float g, float& p, float& m, float& v) {
    m = m * t.beta1 + (1.0f - t.beta1) * g;
    v = v * t.beta2 + (1.0f - t.beta2) * g * g;
    p -= t.step_size * (m / (sqrtf(v) + t.eps));
    if (t.decay > 0.f) p -= t.decay * p;
}

__global__ __launch_bounds__(256) void adamw_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                    const int32_t* __restrict__ chunk_tensor,
                                                    const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                    const float* __restrict__ state, int skip) {
    float coef;
    if (!grad_state(state, skip, coef)) return;
    const Chunk c = chunk_of_block(tab, chunk_tensor, chunk_off, chunk_elems);
    walk<P | G | M | V, P | M | V, ALIGN_ALL>(
        c, coef, [&](int, float& p, float g, float& m, float& v) { adamw_element(c.t, g, p, m, v); });
}

// One element of the RAdam step, in the reference's order: second moment, first moment, decay on the OLD value, then the
// adaptive step (rectified) or the momentum step. `g` arrives already scaled.
__device__ __forceinline__ void radam_element(const vbo_radam_scalars& h, float g, float& p, float& m, float& v) {
    v = v * h.beta2 + h.one_minus_beta2 * g * g;
    m = m * h.beta1 + h.one_minus_beta1 * g;
    if (h.decay != 0.f) p -= h.decay * p;
    if (h.rectified) p -= h.step_size * (m / (sqrtf(v) + h.eps));
    else p -= h.step_size * m;
}

__global__ __launch_bounds__(256) void radam_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                    const vbo_radam_scalars* __restrict__ scalars,
                                                    const int32_t* __restrict__ chunk_tensor,
                                                    const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                    const float* __restrict__ state, int skip) {
    float coef;
    if (!grad_state(state, skip, coef)) return;
    const Chunk c = chunk_of_block(tab, chunk_tensor, chunk_off, chunk_elems);
    const vbo_radam_scalars h = scalars[c.ti];
    walk<P | G | M | V, P | M | V, ALIGN_ALL>(
        c, coef, [&](int, float& p, float g, float& m, float& v) { radam_element(h, g, p, m, v); });
}

// Sum of squares of one chunk of one gradient: per-lane chains of at most chunk_elems / 1024 = 64 fused multiply-adds (fmaf
// spelled out: the unrolled loop keeps them fused in every lane), then the fixed order of optim_walk.h.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                         const int32_t* __restrict__ chunk_tensor,
                                                         const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                         float* __restrict__ partials) {
    const Chunk c = chunk_of_block(tab, chunk_tensor, chunk_off, chunk_elems);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    walk<G, 0, ALIGN_GRAD, 4>(c, 1.0f, [&](int lane, float&, float g, float&, float&) { acc[lane] = fmaf(g, g, acc[lane]); });
    block_sum({lane_sum(acc)}, partials + blockIdx.x);
}

// partials -> state. Thread t adds partials[t], partials[t + 256], ... in index order, then a fixed binary tree over the 256
// threads, all in double. The sum of squares is stored as fp32: it is non-finite exactly when a gradient element is inf / NaN
// or when finite gradients overflow fp32 in the square or in a chunk's sum - both count as an overflowed step.
__global__ __launch_bounds__(256) void grad_norm_finish_kernel(const float* __restrict__ partials, int n, float max_norm,
                                                               float grad_scale, int skip, float* __restrict__ state) {
    __shared__ double tree[256];
    double a = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) a += (double)partials[i];
    tree[threadIdx.x] = a;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) tree[threadIdx.x] += tree[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double ss = tree[0];
        const float ssf = (float)ss;
        const bool finite = isfinite(ssf);
        // the norm of the gradients the step applies (g * grad_scale); coefficient of torch.nn.utils.clip_grad_norm_
        const double norm = fabs((double)grad_scale) * sqrt(ss);
        double clip = 1.0;
        if (max_norm > 0.f) {
            clip = (double)max_norm / (norm + 1e-6);
            if (clip > 1.0) clip = 1.0;          // (a NaN norm stays a NaN coefficient, as torch.clamp keeps it)
        }
        state[VB_GRAD_STATE_SUMSQ] = ssf;
        state[VB_GRAD_STATE_NORM] = (float)norm;
        state[VB_GRAD_STATE_COEF] = (float)((double)grad_scale * clip);
        state[VB_GRAD_STATE_FINITE] = finite ? 1.f : 0.f;
        if (skip && !finite) state[VB_GRAD_STATE_SKIPPED] += 1.f;
    }
}

}  // namespace

// `state` == nullptr is the plain step
static int launch_adamw(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const int32_t* chunk_tensor,
                        const int64_t* chunk_off, int32_t chunk_elems, const float* state, int32_t skip_nonfinite) {
    if (int e = check_tables(n_chunks, table, chunk_tensor, chunk_off, chunk_elems)) return e;
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), table,
                       chunk_tensor, chunk_off, chunk_elems, state, skip_nonfinite != 0 ? 1 : 0);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_adamw_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table,
                             const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems) {
    return launch_adamw(stream, n_chunks, table, chunk_tensor, chunk_off, chunk_elems, nullptr, 0);
}

extern "C" int vbx_adamw_step_scaled(void* stream, int32_t n_chunks, const vb_adamw_tensor* table,
                                     const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems,
                                     const float* state, int32_t skip_nonfinite) {
    if (state == nullptr) return VB_E_BADARG;
    return launch_adamw(stream, n_chunks, table, chunk_tensor, chunk_off, chunk_elems, state, skip_nonfinite);
}

extern "C" int64_t vbx_grad_norm_workspace(int32_t n_chunks) { return n_chunks > 0 ? (int64_t)n_chunks : 0; }

extern "C" int vbx_grad_norm(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const int32_t* chunk_tensor,
                             const int64_t* chunk_off, int32_t chunk_elems, float max_norm, float grad_scale,
                             int32_t skip_nonfinite, float* partials, float* state) {
    if (!(max_norm >= 0.f) || !std::isfinite(max_norm) || !std::isfinite(grad_scale)) return VB_E_BADARG;
    if (int e = check_tables(n_chunks, table, chunk_tensor, chunk_off, chunk_elems, {partials, state})) return e;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, table, chunk_tensor, chunk_off,
                       chunk_elems, partials);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, partials, n_chunks, max_norm, grad_scale,
                       skip_nonfinite != 0, state);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbo_radam_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const vbo_radam_scalars* scalars,
                              const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems, const float* state,
                              int32_t skip_nonfinite) {
    if (int e = check_tables(n_chunks, table, chunk_tensor, chunk_off, chunk_elems, {scalars})) return e;
    hipLaunchKernelGGL(radam_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), table, scalars,
                       chunk_tensor, chunk_off, chunk_elems, state, skip_nonfinite != 0 ? 1 : 0);
    VB_LAUNCH_CHECK();
    return 0;
}
