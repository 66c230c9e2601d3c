/* vilbert_hip_ext.h - entry points added to libvilbert_hip.so after the export list of ABI 18 was frozen.
 *
 * vilbert_hip.h and its `vb_` symbols are pinned name by name (tests/test_abi.py: header, ctypes mirror and `nm -D` must list
 * exactly the ABI-18 set), so additive entry points live here under the prefix `vbx_`. Same conventions as vilbert_hip.h:
 * C linkage, device pointers, `stream` is a hipStream_t passed as void*, every call only enqueues work on it (no allocation,
 * no synchronisation, graph-capture safe), return 0 = ok, > 0 = hipError_t from the launch, < 0 = VB_E_* argument error.
 * The ctypes mirror is vilbert/_native.py: EXT_SIGNATURES (checked against this text by tests/test_optim_clip.py). */
#ifndef VILBERT_HIP_EXT_H
#define VILBERT_HIP_EXT_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Global-norm gradient clipping, gradient scale and overflow-safe AdamW step, all on the device.
 *
 * The three calls take the launch tables of vb_adamw_step (table / chunk_tensor / chunk_off / chunk_elems), so the norm
 * covers exactly the tensors the step updates. Per step:  vbx_grad_norm(...);  vbx_adamw_step_scaled(...).
 *
 * vbx_grad_norm: one block per chunk writes the fp32 sum of squares of its gradient elements to partials[chunk] (16-byte
 * loads where the gradient pointer is 16-byte aligned, scalar loads otherwise; no atomics); one more block adds the
 * partials in index order in double and writes `state` (VB_GRAD_STATE_FLOATS floats, zero-filled by the caller once):
 *   [VB_GRAD_STATE_SUMSQ]   sum of g^2 over every listed gradient (fp32)
 *   [VB_GRAD_STATE_NORM]    |grad_scale| * sqrt(sum): the norm of the gradients the step applies
 *   [VB_GRAD_STATE_COEF]    grad_scale * min(1, max_norm / (norm + 1e-6)) if max_norm > 0 (the coefficient of
 *                           torch.nn.utils.clip_grad_norm_), else grad_scale
 *   [VB_GRAD_STATE_FINITE]  1 if the fp32 sum of squares is finite, else 0. It is not finite exactly when some gradient
 *                           element is inf / NaN, or when finite gradients overflow fp32 in the square or in a chunk's
 *                           sum (|g| > ~1.8e19): both count as an overflowed step
 *   [VB_GRAD_STATE_SKIPPED] += 1 when skip_nonfinite != 0 and FINITE == 0 (a count of skipped steps, exact to 2^24)
 * The summation order is fixed: two calls on the same gradients write the same bits.
 * max_norm < 0 or NaN / inf, grad_scale NaN / inf: VB_E_BADARG.
 *
 * vbx_adamw_step_scaled: vb_adamw_step with every gradient multiplied by state[VB_GRAD_STATE_COEF] as it is loaded. With
 * skip_nonfinite != 0 and state[VB_GRAD_STATE_FINITE] == 0 nothing is stored: parameters and both moments keep their bits.
 * The gradients are only read, never rewritten (apex's FusedAdam takes its scale the same way; clip_grad_norm_ scales the
 * .grad tensors in place).
 * ------------------------------------------------------------------------------------------ */
#define VB_GRAD_STATE_FLOATS  8
#define VB_GRAD_STATE_SUMSQ   0
#define VB_GRAD_STATE_NORM    1
#define VB_GRAD_STATE_COEF    2
#define VB_GRAD_STATE_FINITE  3
#define VB_GRAD_STATE_SKIPPED 4

/* number of floats vbx_grad_norm needs in `partials` */
int64_t vbx_grad_norm_workspace(int32_t n_chunks);

int vbx_grad_norm(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const int32_t* chunk_tensor,
                  const int64_t* chunk_off, int32_t chunk_elems, float max_norm, float grad_scale, int32_t skip_nonfinite,
                  float* partials, float* state);

int vbx_adamw_step_scaled(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const int32_t* chunk_tensor,
                          const int64_t* chunk_off, int32_t chunk_elems, const float* state, int32_t skip_nonfinite);

#ifdef __cplusplus
}
#endif
#endif
