/* vilbert_hip_baseline.h - the single-stream baseline model (vilbert/basebert.py) in libvilbert_hip.so: the joint text + image
 * embedding that writes both segments into one [B, T + R, H] buffer, its backward, the table scatter with the baseline's
 * padding rows, and the tanh of the pooler.
 *
 * The export lists of the other headers (`vb_`, `vbx_`, `vbo_`, `vbt_`, ...) are pinned name by name, so these entry points live
 * here under the prefix `vbb_`. Same conventions as vilbert_hip_tasks.h: C linkage, device pointers, `stream` is a hipStream_t
 * passed as void*, every call only enqueues work on it (no allocation, no synchronisation, graph-capture safe), return
 * 0 = ok, > 0 = hipError_t from the launch, < 0 = VB_E_* argument error, checked before anything is launched. The ctypes
 * mirror is vilbert/_native.py: BASELINE_SIGNATURES (checked against this text by tests/test_basebert.py).
 *
 * Row layout and the LayerNorm are those of vb_text_embed_ln_fwd / vb_image_embed_ln_fwd (one wave per row, TF style: biased
 * variance, eps inside the root). Sample b owns the rows b * (n_tok + n_reg) ... of the joint tensors: its n_tok text rows
 * first, then its n_reg image rows. Common errors: a NULL required pointer, batch < 0 or another size <= 0: VB_E_BADARG;
 * hidden not a multiple of 4 or a pointer read with 16-byte loads not 16-byte aligned: VB_E_ALIGN; hidden > VB_MAX_LN_COLS or
 * batch * (n_tok + n_reg) * hidden beyond int64: VB_E_RANGE. batch == 0 launches nothing, writes nothing and returns 0. */
#ifndef VILBERT_HIP_BASELINE_H
#define VILBERT_HIP_BASELINE_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * One launch over batch * (n_tok + n_reg) rows.
 *   text row j < n_tok:   presum = word[ids[b, j]] + pos[j] + type_t[seg[b, j]], LayerNorm with gamma_t / beta_t; an id
 *                         outside its table contributes a zero row (as in vb_text_embed_ln_fwd);
 *   image row j >= n_tok: presum = feat_proj[b * n_reg + j - n_tok] + type_row + (loc . w_loc^T + b_loc), LayerNorm with
 *                         gamma_v / beta_v; feat_proj [batch * n_reg, hidden] is the feature projection with its bias,
 *                         loc [batch * n_reg, 5], w_loc [hidden, 5], type_row one [hidden] row (the model passes row 1 of
 *                         the image token-type table).
 * Outputs: out [batch, n_tok + n_reg, hidden]; mean / rstd [batch * (n_tok + n_reg)] and presum (same shape as out), each
 * optional (NULL = not wanted); add_mask [batch, n_tok + n_reg] = (1 - m) * -10000 with m from mask_t [batch, n_tok] on the
 * text rows and mask_v [batch, n_reg] on the image rows - each mask int64 (flag 0) or fp32 (flag != 0) as in
 * vb_additive_mask, a NULL mask = all ones.
 * ------------------------------------------------------------------------------------------ */
int vbb_joint_embed_fwd(void* stream, int32_t batch, int32_t n_tok, int32_t n_reg, int32_t hidden, int32_t vocab,
                        int32_t n_types, const int64_t* ids, const int64_t* seg, const float* word_emb, const float* pos_emb,
                        const float* type_emb, const float* gamma_t, const float* beta_t, const float* feat_proj,
                        const float* loc, const float* w_loc, const float* b_loc, const float* type_row,
                        const float* gamma_v, const float* beta_v, float eps, const void* mask_t, int32_t mask_t_is_f32,
                        const void* mask_v, int32_t mask_v_is_f32, float* out, float* mean, float* rstd, float* presum,
                        float* add_mask);

/* ------------------------------------------------------------------------------------------
 * Backward of the two LayerNorms of the joint embedding. dy, presum [batch, n_tok + n_reg, hidden] and mean / rstd are the
 * forward's; dx_text [batch * n_tok, hidden] and dx_img [batch * n_reg, hidden] receive the gradient of the pre-LayerNorm
 * sums, each contiguous (what vbb_text_embed_bwd and the weight-gradient GEMMs of the two image projections consume);
 * dgamma_t / dbeta_t / dgamma_v / dbeta_v [hidden] are OVERWRITTEN with the column sums of their segment.
 * Deterministic: stage 1 stores one partial row per block (per row for hidden > 1024) of ONE segment into `workspace`
 * (vbb_joint_embed_bwd_workspace floats; every element read is written first, so its previous content does not matter),
 * stage 2 adds the partials of a segment in a fixed order. No floating-point atomics: bit-identical from run to run.
 * ------------------------------------------------------------------------------------------ */
int64_t vbb_joint_embed_bwd_workspace(int32_t batch, int32_t n_tok, int32_t n_reg, int32_t hidden);

int vbb_joint_embed_bwd(void* stream, int32_t batch, int32_t n_tok, int32_t n_reg, int32_t hidden, const float* dy,
                        const float* presum, const float* mean, const float* rstd, const float* gamma_t,
                        const float* gamma_v, float* dx_text, float* dx_img, float* dgamma_t, float* dbeta_t,
                        float* dgamma_v, float* dbeta_v, float* workspace);

/* ------------------------------------------------------------------------------------------
 * vb_text_embed_bwd (same arguments, same ordered reduction under the deterministic setting, same counted fallback to the
 * atomic kernels) with the baseline's padding rows: its three text tables are built with padding_idx = 0, so the gather
 * leaves position row 0 (skip_pos0 != 0) and token-type row 0 (skip_type0 != 0) without gradient, like word row 0. A skipped
 * row is never touched - nothing is zeroed after the fact, so accumulating micro-batches into the same tables keeps working.
 * With both flags 0 the call IS vb_text_embed_bwd, bit for bit.
 * ------------------------------------------------------------------------------------------ */
int vbb_text_embed_bwd(void* stream, int32_t batch, int32_t n_tok, int32_t hidden, int32_t vocab, int32_t n_types,
                       int32_t n_tasks, const int64_t* ids, const int64_t* seg, const int64_t* task_ids, const float* dx,
                       float* dword, float* dpos, float* dtype, float* dtask, int32_t skip_pos0, int32_t skip_type0);

/* ------------------------------------------------------------------------------------------
 * The pooler's activation on its [B, H] output: y = tanh(x); dx = dy * (1 - y * y). Elementwise over n values, y may be x
 * and dx may be dy. NULL pointer or n < 0: VB_E_BADARG; n == 0 launches nothing.
 * ------------------------------------------------------------------------------------------ */
int vbb_tanh_fwd(void* stream, int64_t n, const float* x, float* y);

int vbb_tanh_bwd(void* stream, int64_t n, const float* dy, const float* y, float* dx);

#ifdef __cplusplus
}
#endif
#endif
