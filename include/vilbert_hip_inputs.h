/* vilbert_hip_inputs.h - device-side masking of a pre-training batch in libvilbert_hip.so: which tokens and regions a step
 * predicts is drawn on the device from one seed (dynamic masking), for sources that keep UNMASKED samples.
 *
 * The export lists of the other headers are pinned name by name by their tests, so the input side lives here under the prefix
 * `vbi_`. Same conventions as those headers: C linkage, device pointers, `stream` is a hipStream_t passed as void*, every call
 * only enqueues work on it (no allocation, no synchronisation, graph-capture safe), return 0 = ok, > 0 = hipError_t from the
 * launch, < 0 = VB_E_* argument error, checked before anything is launched. The ctypes mirror is vilbert/_native.py:
 * INPUT_SIGNATURES / MaskArgs (checked against this text by tests/test_mask_batch.py); the arithmetic below is restated in
 * numpy by tests/masking_restatement.py, and the kernels are held to it bit for bit (tests/test_mask_batch_gpu.py). */
#ifndef VILBERT_HIP_INPUTS_H
#define VILBERT_HIP_INPUTS_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * MLM and region masking of one batch, ONE launch (one wave per sample). The per-site rule and the probabilities are those of
 * the reference's BertPreprocessBatch.random_word / random_region; the draws are this library's counter-based hash, NOT
 * Python's `random` stream.
 *
 * One uniform per site: u(idx) = float(vb_hash(seed, idx) >> 8) * 2^-24 (csrc/rng.h), idx = (b * 3 + s) * L + pos with
 * L = max(tokens, regions): stream s = 0 is the token draw, s = 1 the replacement token, s = 2 the region draw - disjoint
 * index ranges of the one seed.
 *
 * Tokens, len = sum(input_mask[b, :]): position t is eligible for 1 <= t <= len - 2 ([CLS], [SEP] and padding never are) and
 * selected when u < p_select. With v = u / p_select (fp32 division):
 *     v < 0.8f                      out_input_ids[b, t] = mask_token_id
 *     v < 0.9f                      out_input_ids[b, t] = (uint64(vb_hash(seed, idx of stream 1)) * vocab_size) >> 32
 *     else                          out_input_ids[b, t] = input_ids[b, t]
 *     lm_label_ids[b, t] = input_ids[b, t] at a selected position, -1 everywhere else. out_input_ids may BE input_ids.
 * Regions, boxes = sum(image_mask[b, :]): region i is eligible for i < boxes and selected when u < p_select:
 *     image_label[b, i]  = 1 at a selected region, -1 everywhere else (padding too)
 *     zero_row[b, i]     = 1 where selected and v < 0.9f (the feature row vbi_zero_rows clears), else 0
 *     masked_label[b, j] = 1 iff some selected i has overlaps[b, i, j] > 0.4f, else 0           (j over all `regions`)
 * Every element of the five outputs is written. No atomics: the same inputs give the same bits.
 *
 * Errors: NULL args or a NULL pointer in it, batch < 0, tokens <= 0, regions <= 0, vocab_size <= 0, mask_token_id outside
 * [0, vocab_size), p_select outside [0, 1] or NaN: VB_E_BADARG; 4 * batch * regions * regions (the bytes of overlaps)
 * beyond int64: VB_E_RANGE. batch == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct vbi_mask_args {
    int32_t batch, tokens, regions;
    int32_t vocab_size;
    int32_t mask_token_id;
    float p_select;                 /* the reference's 0.15 */
    uint64_t seed;
    const int64_t* input_ids;       /* [batch, tokens] unmasked: [CLS] ... [SEP], zero padding */
    const int64_t* input_mask;      /* [batch, tokens] */
    const int64_t* image_mask;      /* [batch, regions] */
    const float* overlaps;          /* [batch, regions, regions] IoU of the boxes, zero-padded */
    int64_t* out_input_ids;         /* [batch, tokens] */
    int64_t* lm_label_ids;          /* [batch, tokens] */
    int64_t* image_label;           /* [batch, regions] */
    int64_t* masked_label;          /* [batch, regions] */
    uint8_t* zero_row;              /* [batch, regions] */
} vbi_mask_args;                    /* 104 bytes */

int vbi_concap_mask_batch(void* stream, const vbi_mask_args* args);

/* ------------------------------------------------------------------------------------------
 * Clear the flagged rows of a [rows, n] fp32 matrix (row stride ldx elements), one launch, 16-byte accesses.
 *     out == NULL    in place: the rows with flags[r] != 0 of x become zeros; no other byte of x is read or written
 *     out != NULL    every row of out (row stride ldo) is written: zeros where flags[r] != 0 (x is not read there), the row
 *                    of x otherwise; x is only read. out == x is refused.
 * Elements between n and the row stride are never touched.
 * Errors: NULL x / flags, rows < 0, n <= 0, a row stride < n, out == x: VB_E_BADARG; x or out not 16-byte aligned, n or a row
 * stride not a multiple of 4: VB_E_ALIGN; 4 * rows * stride (a byte offset) beyond int64: VB_E_RANGE. rows == 0 launches
 * nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
int vbi_zero_rows(void* stream, int64_t rows, int32_t n, float* x, int64_t ldx, const uint8_t* flags, float* out, int64_t ldo);

#ifdef __cplusplus
}
#endif
#endif
