/* vilbert_hip_tasks.h - loss and answer score of the fine-tuning heads in libvilbert_hip.so.
 *
 * The export lists of vilbert_hip.h (`vb_`, ABI 18), vilbert_hip_ext.h (`vbx_`) and vilbert_hip_optim.h (`vbo_`) are pinned
 * name by name (tests/test_abi.py, tests/test_optim_clip.py, tests/test_radam.py), so the task-side entry points live here
 * under the prefix `vbt_`. Same conventions as the other headers: C linkage, device pointers, `stream` is a hipStream_t
 * passed as void*, every call only enqueues work on it (no allocation, no synchronisation, graph-capture safe), return
 * 0 = ok, > 0 = hipError_t from the launch, < 0 = VB_E_* argument error, checked before anything is launched. The ctypes
 * mirror is vilbert/_native.py: TASK_SIGNATURES (checked against this text by tests/test_task_losses.py).
 *
 * Every tensor is a [rows, n] fp32 view with contiguous rows and its own row stride in elements (ld* >= n) - the head
 * outputs are views of padded buffers, as with vb_xent_*; a [B, R, 1] region logit is the view [B, R]. Common errors:
 * a NULL required pointer, rows < 0, n <= 0 or a row stride < n: VB_E_BADARG; rows * stride beyond int64: VB_E_RANGE.
 * rows == 0 launches nothing, writes nothing and returns 0. */
#ifndef VILBERT_HIP_TASKS_H
#define VILBERT_HIP_TASKS_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * nn.BCEWithLogitsLoss(reduction="mean"), the loss of eight of the twelve fine-tuning tasks:
 *     loss[0] = (1 / (rows * n)) * sum over r, j of  max(x, 0) - x * t + log1p(exp(-|x|))
 * (the form that overflows at no x). Deterministic: no floating-point atomics - each block of the first launch stores one
 * partial sum into `workspace` (vbt_bce_workspace(rows, n) floats, never more than 1024), a one-block second launch adds
 * them in index order; an input one block covers is finished by the first launch. Bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
int64_t vbt_bce_workspace(int64_t rows, int32_t n);

int vbt_bce_fwd(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const float* target, int64_t ldt,
                float* workspace, float* loss);

/* dlogits[r, j] = (sigmoid(x) - t) * grad_loss[0] / (rows * n), one launch; grad_loss is a device scalar. sigmoid is
 * evaluated from exp(-|x|) and overflows at no x. Row stride of the output: ldd >= n; elements between n and ldd are
 * not touched. */
int vbt_bce_bwd(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const float* target, int64_t ldt,
                const float* grad_loss, float* dlogits, int64_t ldd);

/* ------------------------------------------------------------------------------------------
 * The arithmetic of compute_score_with_logits, one launch: idx[r] = the LOWEST index of the maximum of logits[r, :], a NaN
 * counting as the maximum (torch.max's order); picked[r] = labels[r, idx[r]]. `dense` is optional (NULL = not wanted): the
 * [rows, n] matrix the reference returns (row stride ldo >= n), 0 everywhere and labels[r, idx[r]] at idx[r]; all rows * n
 * elements of it are written, so it needs no clearing. rows > 2^31 - 1: VB_E_RANGE.
 * ------------------------------------------------------------------------------------------ */
int vbt_argmax_pick(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const float* labels, int64_t ldl,
                    int64_t* idx, float* picked, float* dense, int64_t ldo);

#ifdef __cplusplus
}
#endif
#endif
