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
//   adamw_kernel<true>       the update with every gradient multiplied by coef on load; no store at all when the step is skipped
// No atomics and a fixed summation order everywhere: the same gradients give the same bits. The coefficient never visits the
// host, so the three launches are graph-capturable. The gradients themselves are only read.
//
// Multi-tensor RAdam step (vilbert_hip_optim.h; the reference's vilbert/optimization.py:55-98, `--optim RAdam` of train_tasks.py):
//   radam_kernel             the same chunk walk over the same tables; the per-tensor hyper-parameters - step size, rectified
//                            flag, lr * wd - come from a table of their own the host computes in double, the optional state of
//                            grad_norm_finish_kernel scales the gradients and skips an overflowed step as in adamw_kernel<true>
#include <cmath>

#include "common.h"
#include "../../include/vilbert_hip_optim.h"

namespace {

// SCALED = false is the plain step (vb_adamw_step; `state` / `skip` unused). SCALED = true reads the coefficient and the
// finite flag once per block from the state grad_norm_finish_kernel wrote and multiplies every gradient by it on load; a block
// of a skipped step returns before any store.
template <bool SCALED>
__global__ __launch_bounds__(256) void adamw_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                    const int32_t* __restrict__ chunk_tensor,
                                                    const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                    const float* __restrict__ state, int skip) {
    float coef = 1.0f;
    if constexpr (SCALED) {
        if (skip && state[VB_GRAD_STATE_FINITE] == 0.f) return;
        coef = state[VB_GRAD_STATE_COEF];
    }
    const vb_adamw_tensor t = tab[chunk_tensor[blockIdx.x]];
    const long off = chunk_off[blockIdx.x];
    const long end = min((long)t.numel, off + chunk_elems);
    const float b1 = t.beta1, b2 = t.beta2, c1 = 1.0f - t.beta1, c2 = 1.0f - t.beta2;
    float* __restrict__ p = t.param;
    const float* __restrict__ g = t.grad;
    float* __restrict__ m = t.exp_avg;
    float* __restrict__ v = t.exp_avg_sq;
    // 16-byte accesses need all four base pointers 16-byte aligned (chunk offsets are multiples of 4 elements);
    // a tensor that is an oddly offset view takes the scalar loop for its whole chunk
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                          reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    const long n4 = vec_ok ? (end - off) >> 2 : 0;
    for (long i = threadIdx.x; i < n4; i += 256) {
        const long e = off + 4 * i;
        f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
        f32x4 gg = *reinterpret_cast<const f32x4*>(g + e);
        if constexpr (SCALED) gg *= coef;
        f32x4 mm = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            mm[k] = mm[k] * b1 + c1 * gg[k];
            vv[k] = vv[k] * b2 + c2 * gg[k] * gg[k];
            pp[k] -= t.step_size * (mm[k] / (sqrtf(vv[k]) + t.eps));
            if (t.decay > 0.f) pp[k] -= t.decay * pp[k];
        }
        *reinterpret_cast<f32x4*>(p + e) = pp;
        *reinterpret_cast<f32x4*>(m + e) = mm;
        *reinterpret_cast<f32x4*>(v + e) = vv;
    }
    for (long e = off + 4 * n4 + threadIdx.x; e < end; e += 256) {
        float gg = g[e];
        if constexpr (SCALED) gg *= coef;
        const float mm = m[e] * b1 + c1 * gg, vv = v[e] * b2 + c2 * gg * gg;
        float pp = p[e] - t.step_size * (mm / (sqrtf(vv) + t.eps));
        if (t.decay > 0.f) pp -= t.decay * pp;
        p[e] = pp; m[e] = mm; v[e] = vv;
    }
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

// `state` == nullptr is the plain step; otherwise the coefficient and the finite flag are read once per block (uniform
// branches) and a block of a skipped step returns before any store. coef = 1 multiplies exactly, so one kernel serves both.
__global__ __launch_bounds__(256) void radam_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                    const vbo_radam_scalars* __restrict__ scalars,
                                                    const int32_t* __restrict__ chunk_tensor,
                                                    const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                    const float* __restrict__ state, int skip) {
    float coef = 1.0f;
    if (state != nullptr) {
        if (skip && state[VB_GRAD_STATE_FINITE] == 0.f) return;
        coef = state[VB_GRAD_STATE_COEF];
    }
    const int ti = chunk_tensor[blockIdx.x];
    const vb_adamw_tensor t = tab[ti];
    const vbo_radam_scalars h = scalars[ti];
    const long off = chunk_off[blockIdx.x];
    const long end = min((long)t.numel, off + chunk_elems);
    float* __restrict__ p = t.param;
    const float* __restrict__ g = t.grad;
    float* __restrict__ m = t.exp_avg;
    float* __restrict__ v = t.exp_avg_sq;
    // as adamw_kernel: 16-byte accesses only where all four base pointers allow them (chunk offsets are multiples of 4)
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                          reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    const long n4 = vec_ok ? (end - off) >> 2 : 0;
    for (long i = threadIdx.x; i < n4; i += 256) {
        const long e = off + 4 * i;
        f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e) * coef;
        f32x4 mm = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], mk = mm[k], vk = vv[k];
            radam_element(h, gg[k], pk, mk, vk);
            pp[k] = pk; mm[k] = mk; vv[k] = vk;
        }
        *reinterpret_cast<f32x4*>(p + e) = pp;
        *reinterpret_cast<f32x4*>(m + e) = mm;
        *reinterpret_cast<f32x4*>(v + e) = vv;
    }
    for (long e = off + 4 * n4 + threadIdx.x; e < end; e += 256) {
        float pp = p[e], mm = m[e], vv = v[e];
        radam_element(h, g[e] * coef, pp, mm, vv);
        p[e] = pp; m[e] = mm; v[e] = vv;
    }
}

// Sum of squares of one chunk of one gradient. Fixed order: four per-thread accumulators (one per vector lane; the scalar
// path uses the first), each a chain of at most chunk_elems / 1024 = 64 adds, combined lane 0..3, then the xor tree of the
// wave, then waves 0..3 through LDS.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                         const int32_t* __restrict__ chunk_tensor,
                                                         const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                         float* __restrict__ partials) {
    const int ti = chunk_tensor[blockIdx.x];
    const float* __restrict__ g = tab[ti].grad;
    const long off = chunk_off[blockIdx.x];
    const long end = min((long)tab[ti].numel, off + chunk_elems);
    const bool vec_ok = (reinterpret_cast<uintptr_t>(g) & 15u) == 0;
    const long n4 = vec_ok ? (end - off) >> 2 : 0;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (long i = threadIdx.x; i < n4; i += 256) {
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + off + 4 * i);
        acc += gg * gg;
    }
    for (long e = off + 4 * n4 + threadIdx.x; e < end; e += 256) acc[0] += g[e] * g[e];
    const float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    __shared__ float wave_part[4];
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = (wave_part[0] + wave_part[1]) + (wave_part[2] + wave_part[3]);
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

extern "C" int vb_adamw_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table,
                             const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems) {
    if (table == nullptr || chunk_tensor == nullptr || chunk_off == nullptr || n_chunks <= 0) return VB_E_BADARG;
    if (chunk_elems <= 0 || chunk_elems % 4 != 0) return VB_E_ALIGN;
    hipLaunchKernelGGL(adamw_kernel<false>, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), table,
                       chunk_tensor, chunk_off, chunk_elems, static_cast<const float*>(nullptr), 0);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vbx_grad_norm_workspace(int32_t n_chunks) { return n_chunks > 0 ? (int64_t)n_chunks : 0; }

extern "C" int vbx_grad_norm(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const int32_t* chunk_tensor,
                             const int64_t* chunk_off, int32_t chunk_elems, float max_norm, float grad_scale,
                             int32_t skip_nonfinite, float* partials, float* state) {
    if (table == nullptr || chunk_tensor == nullptr || chunk_off == nullptr || partials == nullptr || state == nullptr ||
        n_chunks <= 0)
        return VB_E_BADARG;
    if (!(max_norm >= 0.f) || !std::isfinite(max_norm) || !std::isfinite(grad_scale)) return VB_E_BADARG;
    if (chunk_elems <= 0 || chunk_elems % 4 != 0) return VB_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, table, chunk_tensor, chunk_off,
                       chunk_elems, partials);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, st, partials, n_chunks, max_norm, grad_scale,
                       skip_nonfinite != 0, state);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbx_adamw_step_scaled(void* stream, int32_t n_chunks, const vb_adamw_tensor* table,
                                     const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems,
                                     const float* state, int32_t skip_nonfinite) {
    if (table == nullptr || chunk_tensor == nullptr || chunk_off == nullptr || state == nullptr || n_chunks <= 0)
        return VB_E_BADARG;
    if (chunk_elems <= 0 || chunk_elems % 4 != 0) return VB_E_ALIGN;
    hipLaunchKernelGGL(adamw_kernel<true>, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), table,
                       chunk_tensor, chunk_off, chunk_elems, state, skip_nonfinite != 0 ? 1 : 0);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbo_radam_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const vbo_radam_scalars* scalars,
                              const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems, const float* state,
                              int32_t skip_nonfinite) {
    if (table == nullptr || scalars == nullptr || chunk_tensor == nullptr || chunk_off == nullptr || n_chunks <= 0)
        return VB_E_BADARG;
    if (chunk_elems <= 0 || chunk_elems % 4 != 0) return VB_E_ALIGN;
    hipLaunchKernelGGL(radam_kernel, dim3((unsigned)n_chunks), dim3(256), 0, static_cast<hipStream_t>(stream), table, scalars,
                       chunk_tensor, chunk_off, chunk_elems, state, skip_nonfinite != 0 ? 1 : 0);
    VB_LAUNCH_CHECK();
    return 0;
}
