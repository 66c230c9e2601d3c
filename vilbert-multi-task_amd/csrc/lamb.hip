// Multi-tensor LAMB step (vilbert_hip_lamb.h; You et al. 2020): Adam with one trust ratio ||p|| / ||u|| per parameter tensor,
// on the launch tables of adamw_kernel / radam_kernel (optimizer.hip) plus a per-tensor table of host-computed scalars.
//   lamb_stage1_kernel   one block per chunk: g (x coef) -> m, v stored; u formed in registers; the chunk's fp32 partial sums
//                        of p^2 and u^2 -> workspace[chunk][2]                      (16 B read + 8 B written per parameter)
//   lamb_stage2_kernel   the same grid: u recomputed from the stored m, v and the old p (lamb_update, the function stage 1
//                        used); every block sums its tensor's partial pairs in index order in double -> r; p -= lr r u
//                        (12 B read + 4 B written per parameter)
// The gradients are only read (the base class of the optimizers promises that `.grad` is not modified), so u is not parked in
// them; with the norm pass of vbx_grad_norm the step moves 4 + 24 + 16 = 44 B per parameter against 4 + 28 = 32 B of the
// clipped AdamW step. No atomics and a fixed summation order everywhere (that of grad_sumsq_kernel inside a block): a
// tensor's bits depend on its own values, its alignment and the coefficient only - not on where it stands in the tables.
#include <cmath>

#include "common.h"
#include "../../include/vilbert_hip_lamb.h"

namespace {

// The moments of one element: `g` arrives scaled by the clip coefficient; L2 mode adds the decay to it.
__device__ __forceinline__ void lamb_moments(const vbl_lamb_scalars& h, float g, float p, float& m, float& v) {
    if (!h.adam_w_mode) g += h.weight_decay * p;
    m = m * h.beta1 + h.beta3 * g;
    v = v * h.beta2 + h.one_minus_beta2 * g * g;
}

// The update direction of one element from the NEW moments and the OLD parameter - used by both stages, so that the norm
// stage 1 measures is the norm of what stage 2 applies.
__device__ __forceinline__ float lamb_update(const vbl_lamb_scalars& h, float p, float m, float v) {
    float u = (m / h.bc1) / (sqrtf(v / h.bc2) + h.eps);
    if (h.adam_w_mode) u += h.weight_decay * p;
    return u;
}

// block-wide sums of two values in the fixed order of grad_sumsq_kernel: the xor tree of each wave, then waves 0..3 through LDS
__device__ __forceinline__ void block_sum2(float a, float b, float* __restrict__ out) {
    __shared__ float wave_part[2][4];
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) {
        wave_part[0][threadIdx.x >> 6] = a;
        wave_part[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = (wave_part[0][0] + wave_part[0][1]) + (wave_part[0][2] + wave_part[0][3]);
        out[1] = (wave_part[1][0] + wave_part[1][1]) + (wave_part[1][2] + wave_part[1][3]);
    }
}

// `state` == nullptr: coefficient 1, never skipped. A block of a skipped step returns before any store (uniform branch).
__global__ __launch_bounds__(256) void lamb_stage1_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                          const vbl_lamb_scalars* __restrict__ scalars,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                          float* __restrict__ workspace, const float* __restrict__ state,
                                                          int skip) {
    float coef = 1.0f;
    if (state != nullptr) {
        if (skip && state[VB_GRAD_STATE_FINITE] == 0.f) return;
        coef = state[VB_GRAD_STATE_COEF];
    }
    const int ti = chunk_tensor[blockIdx.x];
    const vb_adamw_tensor t = tab[ti];
    const vbl_lamb_scalars h = scalars[ti];
    const long off = chunk_off[blockIdx.x];
    const long end = min((long)t.numel, off + chunk_elems);
    const float* __restrict__ p = t.param;
    const float* __restrict__ g = t.grad;
    float* __restrict__ m = t.exp_avg;
    float* __restrict__ v = t.exp_avg_sq;
    // as adamw_kernel: 16-byte accesses only where all four base pointers allow them (chunk offsets are multiples of 4)
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                          reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    const long n4 = vec_ok ? (end - off) >> 2 : 0;
    // four per-thread accumulators per sum (one per vector lane; the scalar path uses the first), each a chain of at most
    // chunk_elems / 1024 adds
    f32x4 acc_p = {0.f, 0.f, 0.f, 0.f}, acc_u = {0.f, 0.f, 0.f, 0.f};
    for (long i = threadIdx.x; i < n4; i += 256) {
        const long e = off + 4 * i;
        const f32x4 pp = *reinterpret_cast<const f32x4*>(p + e);
        const f32x4 gg = *reinterpret_cast<const f32x4*>(g + e) * coef;
        f32x4 mm = *reinterpret_cast<f32x4*>(m + e), vv = *reinterpret_cast<f32x4*>(v + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float mk = mm[k], vk = vv[k];
            lamb_moments(h, gg[k], pp[k], mk, vk);
            const float u = lamb_update(h, pp[k], mk, vk);
            mm[k] = mk; vv[k] = vk;
            acc_p[k] += pp[k] * pp[k];
            acc_u[k] += u * u;
        }
        *reinterpret_cast<f32x4*>(m + e) = mm;
        *reinterpret_cast<f32x4*>(v + e) = vv;
    }
    for (long e = off + 4 * n4 + threadIdx.x; e < end; e += 256) {
        const float pp = p[e];
        float mm = m[e], vv = v[e];
        lamb_moments(h, g[e] * coef, pp, mm, vv);
        const float u = lamb_update(h, pp, mm, vv);
        m[e] = mm; v[e] = vv;
        acc_p[0] += pp * pp;
        acc_u[0] += u * u;
    }
    block_sum2((acc_p[0] + acc_p[1]) + (acc_p[2] + acc_p[3]), (acc_u[0] + acc_u[1]) + (acc_u[2] + acc_u[3]),
               workspace + 2 * (long)blockIdx.x);
}

__global__ __launch_bounds__(256) void lamb_stage2_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                          const vbl_lamb_scalars* __restrict__ scalars,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                          const float* __restrict__ workspace, float* __restrict__ trust,
                                                          const float* __restrict__ state, int skip) {
    if (state != nullptr && skip && state[VB_GRAD_STATE_FINITE] == 0.f) return;
    const int ti = chunk_tensor[blockIdx.x];
    const vb_adamw_tensor t = tab[ti];
    const vbl_lamb_scalars h = scalars[ti];
    // the tensor's two norms: its partial pairs in index order, in double; block-uniform addresses, every thread the same
    // sum (the largest tensor of the base model has 358 chunks). The range is clamped to the grid: the workspace has one
    // pair per block.
    float r = 1.0f;
    if (h.apply_trust) {
        const int first = max(h.first_chunk, 0), last = min(h.first_chunk + h.n_chunks, (int)gridDim.x);
        double sp = 0.0, su = 0.0;
        for (int c = first; c < last; ++c) {
            sp += (double)workspace[2 * (long)c];
            su += (double)workspace[2 * (long)c + 1];
        }
        const double pn = sqrt(sp), un = sqrt(su);
        if (pn > 0.0 && un > 0.0) r = (float)(pn / un);
    }
    if (threadIdx.x == 0 && (int)blockIdx.x == h.first_chunk) trust[ti] = r;
    const float step = h.lr * r;
    const long off = chunk_off[blockIdx.x];
    const long end = min((long)t.numel, off + chunk_elems);
    float* __restrict__ p = t.param;
    const float* __restrict__ m = t.exp_avg;
    const float* __restrict__ v = t.exp_avg_sq;
    // the gradient pointer takes part in the choice, so that both stages walk a chunk the same way
    const bool vec_ok = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(t.grad) | reinterpret_cast<uintptr_t>(m) |
                          reinterpret_cast<uintptr_t>(v)) & 15u) == 0;
    const long n4 = vec_ok ? (end - off) >> 2 : 0;
    for (long i = threadIdx.x; i < n4; i += 256) {
        const long e = off + 4 * i;
        f32x4 pp = *reinterpret_cast<f32x4*>(p + e);
        const f32x4 mm = *reinterpret_cast<const f32x4*>(m + e), vv = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) pp[k] -= step * lamb_update(h, pp[k], mm[k], vv[k]);
        *reinterpret_cast<f32x4*>(p + e) = pp;
    }
    for (long e = off + 4 * n4 + threadIdx.x; e < end; e += 256) {
        const float pp = p[e];
        p[e] = pp - step * lamb_update(h, pp, m[e], v[e]);
    }
}

}  // namespace

extern "C" int64_t vbl_lamb_workspace(int32_t n_chunks) { return n_chunks > 0 ? 2 * (int64_t)n_chunks : 0; }

extern "C" int vbl_lamb_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const vbl_lamb_scalars* scalars,
                             const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems, float* workspace,
                             float* trust, const float* state, int32_t skip_nonfinite) {
    if (table == nullptr || scalars == nullptr || chunk_tensor == nullptr || chunk_off == nullptr || workspace == nullptr ||
        trust == nullptr || n_chunks <= 0)
        return VB_E_BADARG;
    if (chunk_elems <= 0 || chunk_elems % 4 != 0) return VB_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int skip = skip_nonfinite != 0 ? 1 : 0;
    hipLaunchKernelGGL(lamb_stage1_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, table, scalars, chunk_tensor, chunk_off,
                       chunk_elems, workspace, state, skip);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(lamb_stage2_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, table, scalars, chunk_tensor, chunk_off,
                       chunk_elems, static_cast<const float*>(workspace), trust, state, skip);
    VB_LAUNCH_CHECK();
    return 0;
}
