/* vilbert_hip_lamb.h - the LAMB optimizer step of libvilbert_hip.so (You et al. 2020, "Large Batch Optimization for Deep
 * Learning: Training BERT in 76 minutes"): Adam with one trust ratio ||p|| / ||update|| per parameter tensor.
 *
 * The export lists of the other headers are pinned name by name by their tests, so LAMB lives here under the prefix `vbl_`.
 * Same conventions as those headers: C linkage, device pointers, `stream` is a hipStream_t passed as void*, every call only
 * enqueues work on it (no allocation, no synchronisation, graph-capture safe), return 0 = ok, > 0 = hipError_t from the launch,
 * < 0 = VB_E_* argument error. The ctypes mirror is vilbert/_native.py: LAMB_SIGNATURES / LambScalars (checked against this
 * text by tests/test_lamb.py). */
#ifndef VILBERT_HIP_LAMB_H
#define VILBERT_HIP_LAMB_H

#include "vilbert_hip_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Multi-tensor LAMB step: TWO launches update every tensor.
 *
 * It walks the launch tables of vb_adamw_step: `table` supplies param / grad / exp_avg / exp_avg_sq / numel of each tensor
 * (its hyper-parameter fields are NOT read), chunk_tensor / chunk_off / chunk_elems list the chunks, and the chunks of one
 * tensor are consecutive in that list. The hyper-parameters come from `scalars`, one entry per entry of `table`, computed by
 * the host in double from each tensor's own step count and rounded once to float.
 * Per tensor, in fp32 (g = the gradient times state[VB_GRAD_STATE_COEF] when `state` is given):
 *     g += weight_decay * p                                    if adam_w_mode == 0   (L2 mode)
 *     m = beta1 * m + beta3 * g                                beta3 = 1 - beta1 (grad averaging) or 1
 *     v = beta2 * v + one_minus_beta2 * g * g
 *     u = (m / bc1) / (sqrt(v / bc2) + eps)                    bc = 1 - beta^t (bias correction) or 1
 *     u += weight_decay * p                                    if adam_w_mode != 0   (decoupled decay)
 *     r = ||p|| / ||u||   if apply_trust != 0 and ||p|| > 0 and ||u|| > 0, else 1       (p before the update)
 *     p = p - lr * r * u
 *
 * Stage 1 (one 256-thread block per chunk) reads g, m, v, p, writes m and v and stores the chunk's fp32 partial sums of p^2
 * and u^2 to workspace[2 * chunk], workspace[2 * chunk + 1]: a fixed summation order inside the block, no atomics. Stage 2
 * (the same grid) reads m, v, p, recomputes u with the same device function, sums the n_chunks partial pairs of its tensor in
 * index order in double, forms r and updates p; the block of a tensor's first chunk also stores r to trust[tensor]. The
 * gradients are only read (44 bytes move per parameter together with the norm pass of vbx_grad_norm). The same inputs give
 * the same bits, wherever a tensor stands in the tables.
 *
 * `state` is optional (NULL = coefficient 1, never skipped). When given it is the device state vbx_grad_norm wrote for the
 * SAME tables; with skip_nonfinite != 0 and state[VB_GRAD_STATE_FINITE] == 0 neither stage stores anything: parameters, both
 * moments, the workspace and `trust` keep their bits. 16-byte loads and stores where all four pointers of a tensor are 16-byte
 * aligned, scalar ones otherwise.
 *
 * vbl_lamb_workspace: the size of `workspace` in floats (2 per chunk; 0 for n_chunks <= 0). `trust` holds one float per
 * entry of `table`.
 * Errors: NULL table / scalars / chunk lists / workspace / trust or n_chunks <= 0: VB_E_BADARG; chunk_elems <= 0 or not a
 * multiple of 4: VB_E_ALIGN (as vb_adamw_step).
 * ------------------------------------------------------------------------------------------ */
typedef struct vbl_lamb_scalars {
    float lr;
    float weight_decay;
    float beta1, beta2;
    float beta3;             /* 1 - beta1 rounded from the double, or 1 without gradient averaging */
    float one_minus_beta2;   /* rounded from the double 1 - beta2 */
    float bc1, bc2;          /* 1 - beta^t of the tensor's own step count t, or 1 without bias correction */
    float eps;
    int32_t adam_w_mode;     /* != 0: decoupled decay (added to the update); 0: L2 (added to the gradient) */
    int32_t apply_trust;     /* != 0: scale by ||p|| / ||u||; 0: r = 1 */
    int32_t first_chunk;     /* index of the tensor's first chunk in the chunk lists */
    int32_t n_chunks;        /* number of its chunks (consecutive) */
} vbl_lamb_scalars;          /* 52 bytes */

int64_t vbl_lamb_workspace(int32_t n_chunks);

int vbl_lamb_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const vbl_lamb_scalars* scalars,
                  const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems, float* workspace, float* trust,
                  const float* state, int32_t skip_nonfinite);

#ifdef __cplusplus
}
#endif
#endif
