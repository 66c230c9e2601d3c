// Multi-tensor LAMB step (vilbert_hip_lamb.h; You et al. 2020): Adam with one trust ratio ||p|| / ||u|| per parameter tensor,
// on the launch tables and the chunk walk of the other optimizers (optim_walk.h) plus a per-tensor table of host-computed scalars.
//   lamb_stage1_kernel   one block per chunk: g (x coef) -> m, v stored; u formed in registers; the chunk's fp32 partial sums
//                        of p^2 and u^2 -> workspace[chunk][2]                      (16 B read + 8 B written per parameter)
//   lamb_stage2_kernel   the same grid: u recomputed from the stored m, v and the old p (lamb_update, the function stage 1
//                        used); every block sums its tensor's partial pairs in index order in double -> r; p -= lr r u
//                        (12 B read + 4 B written per parameter)
// The gradients are only read (the base class of the optimizers promises that `.grad` is not modified), so u is not parked in
// them; with the norm pass of vbx_grad_norm the step moves 4 + 24 + 16 = 44 B per parameter against 4 + 28 = 32 B of the
// clipped AdamW step. No atomics and a fixed summation order everywhere (that of optim_walk.h inside a block): a
// tensor's bits depend on its own values, its alignment and the coefficient only - not on where it stands in the tables.
#include <cmath>

#include "optim_walk.h"
#include "../../include/vilbert_hip_lamb.h"

namespace {

using namespace optim_walk;

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

// The moments in the walk's element functor, the two sums in its trailing one (per-lane chains of at most chunk_elems / 1024
// adds per sum): where the accumulation stands decides which multiply-adds of a round the compiler fuses (optim_walk.h).
__global__ __launch_bounds__(256) void lamb_stage1_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                          const vbl_lamb_scalars* __restrict__ scalars,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                          float* __restrict__ workspace, const float* __restrict__ state,
                                                          int skip) {
    float coef;
    if (!grad_state(state, skip, coef)) return;
    const Chunk c = chunk_of_block(tab, chunk_tensor, chunk_off, chunk_elems);
    const vbl_lamb_scalars h = scalars[c.ti];
    f32x4 acc_p = {0.f, 0.f, 0.f, 0.f}, acc_u = {0.f, 0.f, 0.f, 0.f};
    walk<P | G | M | V, M | V, ALIGN_ALL>(
        c, coef, [&](int, float p, float g, float& m, float& v) { lamb_moments(h, g, p, m, v); },
        [&](int lane, float p, float, float m, float v) {
            const float u = lamb_update(h, p, m, v);
            acc_p[lane] += p * p;
            acc_u[lane] += u * u;
        });
    block_sum({lane_sum(acc_p), lane_sum(acc_u)}, workspace + 2 * (long)blockIdx.x);
}

__global__ __launch_bounds__(256) void lamb_stage2_kernel(const vb_adamw_tensor* __restrict__ tab,
                                                          const vbl_lamb_scalars* __restrict__ scalars,
                                                          const int32_t* __restrict__ chunk_tensor,
                                                          const int64_t* __restrict__ chunk_off, int chunk_elems,
                                                          const float* __restrict__ workspace, float* __restrict__ trust,
                                                          const float* __restrict__ state, int skip) {
    float coef;          // (applied by stage 1)
    if (!grad_state(state, skip, coef)) return;
    const Chunk c = chunk_of_block(tab, chunk_tensor, chunk_off, chunk_elems);
    const vbl_lamb_scalars h = scalars[c.ti];
    // the tensor's two norms: its partial pairs in index order, in double; block-uniform addresses, every thread the same
    // sum (the largest tensor of the base model has 358 chunks). The range is clamped to the grid: the workspace has one
    // pair per block.
    float r = 1.0f;
    if (h.apply_trust) {
        const int first = max(h.first_chunk, 0), last = min(h.first_chunk + h.n_chunks, (int)gridDim.x);
        double sp = 0.0, su = 0.0;
        for (int k = first; k < last; ++k) {
            sp += (double)workspace[2 * (long)k];
            su += (double)workspace[2 * (long)k + 1];
        }
        const double pn = sqrt(sp), un = sqrt(su);
        if (pn > 0.0 && un > 0.0) r = (float)(pn / un);
    }
    if (threadIdx.x == 0 && (int)blockIdx.x == h.first_chunk) trust[c.ti] = r;
    const float step = h.lr * r;
    walk<P | M | V, P, ALIGN_ALL>(c, coef, [&](int, float& p, float, float& m, float& v) { p -= step * lamb_update(h, p, m, v); });
}

}  // namespace

extern "C" int64_t vbl_lamb_workspace(int32_t n_chunks) { return n_chunks > 0 ? 2 * (int64_t)n_chunks : 0; }

extern "C" int vbl_lamb_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const vbl_lamb_scalars* scalars,
                             const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems, float* workspace,
                             float* trust, const float* state, int32_t skip_nonfinite) {
    if (int e = check_tables(n_chunks, table, chunk_tensor, chunk_off, chunk_elems, {scalars, workspace, trust})) return e;
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
