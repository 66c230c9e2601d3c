/* vilbert_hip_optim.h - optimizer entry points of libvilbert_hip.so beyond AdamW.
 *
 * The export lists of vilbert_hip.h (`vb_`, ABI 18) and vilbert_hip_ext.h (`vbx_`) are pinned name by name
 * (tests/test_abi.py, tests/test_optim_clip.py), so further optimizers live here under the prefix `vbo_`. Same conventions as
 * the other two headers: C linkage, device pointers, `stream` is a hipStream_t passed as void*, every call only enqueues work
 * on it (no allocation, no synchronisation, graph-capture safe), return 0 = ok, > 0 = hipError_t from the launch, < 0 = VB_E_*
 * argument error. The ctypes mirror is vilbert/_native.py: OPT_SIGNATURES (checked against this text by tests/test_radam.py). */
#ifndef VILBERT_HIP_OPTIM_H
#define VILBERT_HIP_OPTIM_H

#include "vilbert_hip_ext.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Multi-tensor RAdam step (Liu et al. 2019, "On the Variance of the Adaptive Learning Rate and Beyond"), the arithmetic of
 * the `RAdam` / `PlainRAdam` classes the fine-tuning script offers as `--optim RAdam`. ONE launch updates every tensor.
 *
 * It walks the launch tables of vb_adamw_step: `table` supplies param / grad / exp_avg / exp_avg_sq / numel of each tensor
 * (its hyper-parameter fields are NOT read), chunk_tensor / chunk_off / chunk_elems list the chunks. The hyper-parameters come
 * from `scalars`, one entry per entry of `table`, computed by the host in double from each tensor's own step count.
 * Per element, in fp32 and in this order:
 *     v = beta2 * v + one_minus_beta2 * g * g
 *     m = beta1 * m + one_minus_beta1 * g
 *     p -= decay * p                                   if decay != 0       (decay = lr * weight_decay)
 *     p -= step_size * m / (sqrt(v) + eps)             if rectified != 0   (variance of the adaptive rate is tractable)
 *     p -= step_size * m                               otherwise           (the first steps: SGD with momentum)
 * Which of the two classes is meant shows only in the scalars the host fills in: there is one kernel.
 *
 * `state` is optional (NULL = the plain step). When given it is the device state vbx_grad_norm wrote for the SAME tables:
 * every gradient is multiplied by state[VB_GRAD_STATE_COEF] as it is loaded, and with skip_nonfinite != 0 and
 * state[VB_GRAD_STATE_FINITE] == 0 nothing is stored - parameters and both moments keep their bits. The gradients are only
 * read. 16-byte loads and stores where all four pointers of a tensor are 16-byte aligned, scalar ones otherwise; no atomics.
 * Errors: NULL table / scalars / chunk lists or n_chunks <= 0: VB_E_BADARG; chunk_elems <= 0 or not a multiple of 4:
 * VB_E_ALIGN (as vb_adamw_step).
 * ------------------------------------------------------------------------------------------ */
typedef struct vbo_radam_scalars {
    float step_size;         /* lr * rectification / (1 - beta1^t), or lr / (1 - beta1^t) while not rectified */
    float decay;             /* lr * weight_decay; 0 = no decay */
    float beta1, beta2;
    float one_minus_beta1;   /* rounded from the double 1 - beta: (1.0f - beta) in fp32 is off by up to 2^-24 / (1 - beta) */
    float one_minus_beta2;
    float eps;
    int32_t rectified;       /* != 0: adaptive step */
} vbo_radam_scalars;         /* 32 bytes */

int vbo_radam_step(void* stream, int32_t n_chunks, const vb_adamw_tensor* table, const vbo_radam_scalars* scalars,
                   const int32_t* chunk_tensor, const int64_t* chunk_off, int32_t chunk_elems, const float* state,
                   int32_t skip_nonfinite);

#ifdef __cplusplus
}
#endif
#endif
