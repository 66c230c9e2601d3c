/* vilbert_hip_wire.h - half-width region features on the wire, in libvilbert_hip.so: a feature store that keeps the detector's
 * post-ReLU activations as IEEE binary16 hands them over as they are, and the device finishes the batch from the 16-bit rows.
 * The two calls below do the arithmetic of the fp32 finishing calls - the Conceptual-Captions one of vilbert_hip.h
 * (csrc/batch.hip) and the fine-tuning builder of vilbert_hip_task_inputs.h (csrc/task_batch.hip) - on features that are
 * widened to fp32 as they are read, and can write the feature block as bf16 for the bf16 stream, whose first step rounds it to
 * bf16 anyway. Half the bytes cross the bus, 25 % (fp32 out) or 50 % (bf16 out) fewer move through HBM.
 *
 * The export lists of the other headers are pinned name by name by their tests, so this side lives here under the prefix
 * `vbw_`. Same conventions as those headers: C linkage, device pointers, `stream` is a hipStream_t passed as void*, every call
 * only enqueues work on it (no allocation, no synchronisation, no atomics, graph-capture safe), return 0 = ok, > 0 = hipError_t
 * from the launch, < 0 = VB_E_* argument error, checked before anything is launched. The ctypes mirror is vilbert/_native.py:
 * WIRE_SIGNATURES / WireConcapBatch / WireTaskBatch (checked against this text by tests/test_wire16.py); the kernels are held
 * bit for bit to the fp32 calls run on the exactly widened arrays (tests/test_wire16_gpu.py).
 *
 * Number formats. A feature is a uint16_t holding an IEEE binary16. widen(h) is its exact fp32 value: subnormals, signed zeros
 * and infinities keep their value, a NaN stays a NaN. out_kind selects the element type of the feature output:
 *     0   fp32:  the fp32 result as it is
 *     1   bf16:  the fp32 result rounded to nearest even, NaN-safe (csrc/bf16_round.h), stored as uint16_t
 * Every fp32 operation below is a single IEEE operation rounded to nearest: nothing is contracted into a fused multiply-add.
 * The boxes, masks, labels and the IoU target have no 16-bit input: they are written by the kernels of the fp32 calls. */
#ifndef VILBERT_HIP_WIRE_H
#define VILBERT_HIP_WIRE_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBW_OUT_F32 0
#define VBW_OUT_BF16 1

/* ------------------------------------------------------------------------------------------
 * Finishing of a Conceptual-Captions pre-training batch from binary16 features. B = batch, R = regions, T = tokens,
 * F = feat_dim. With x[b, r, :] = zero_row != NULL and zero_row[b, r] != 0 ? zeros : widen(image_feat[b, r, :]):
 *   out_image_feat [B, R + 1, F] (out_kind)
 *     row 0          the fp32 sum of x[b, 0 .. R - 1, :] IN ROW ORDER, divided in fp64 by max(#(masked_label[b, :] == 0), 1)
 *                    and rounded to fp32
 *     rows 1 .. R    x[b, 0 .. R - 1, :]
 *   out_image_loc [B, R + 1, 5], out_image_mask [B, R + 1] int64, out_image_label [B, R], out_lm_label_ids [B, T]: as the
 *   fp32 call writes them (row 0 of the boxes is 0, 0, 1, 1, 1 and of the mask 1; with objective == 1 both label tensors
 *   are multiplied by (is_next == 0) and zeros become -1, otherwise they are copied).
 * zero_row holds the flags of the masking launch (vilbert_hip_inputs.h): a flagged feature row is not read at all - there is
 * no separate row-clearing launch for 16-bit rows, and image_feat is never written. Every element of every output is written.
 *
 * Errors: NULL args, a NULL pointer other than zero_row, batch < 0, regions <= 0, tokens <= 0, feat_dim <= 0, out_kind
 * outside {0, 1}: VB_E_BADARG; feat_dim % 8 != 0, image_feat or out_image_feat not 16-byte aligned: VB_E_ALIGN;
 * 2 * batch * regions * feat_dim or 4 * batch * (regions + 1) * feat_dim (a byte offset) beyond int64: VB_E_RANGE.
 * batch == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct vbw_concap_batch {
    int32_t batch, regions, tokens, feat_dim, objective, out_kind;
    const uint16_t* image_feat;     /* [B, R, F] binary16 */
    const float* image_loc;         /* [B, R, 5] */
    const int64_t* image_mask;      /* [B, R] */
    const int64_t* masked_label;    /* [B, R] */
    const int64_t* is_next;         /* [B] */
    const int64_t* image_label;     /* [B, R] */
    const int64_t* lm_label_ids;    /* [B, T] */
    const uint8_t* zero_row;        /* [B, R] or NULL: no row is flagged */
    void* out_image_feat;           /* [B, R + 1, F] fp32 or bf16 */
    float* out_image_loc;           /* [B, R + 1, 5] */
    int64_t* out_image_mask;        /* [B, R + 1] */
    int64_t* out_image_label;       /* [B, R] */
    int64_t* out_lm_label_ids;      /* [B, T] */
} vbw_concap_batch;                 /* 128 bytes */

int vbw_concap_finish_batch(void* stream, const vbw_concap_batch* args);

/* ------------------------------------------------------------------------------------------
 * Padded inputs of one fine-tuning batch from packed binary16 regions. Sample b owns the packed rows offsets[b] ..
 * offsets[b + 1] - 1 (n_b rows); R = max_regions, kept_b = min(n_b + 1, R). The words of `offsets` and `mean_rows` live on
 * the device and are clamped before any address is formed (csrc/task_rows.h), exactly as the fp32 builder clamps them.
 *   out_feat [batch, R, feat_dim] (out_kind)
 *     row 0                  the fp32 sum of the first count = mean_rows[b] (NULL: n_b) widened packed rows IN ROW ORDER, divided
 *                            in fp32 by (float)count - over all count rows, also where R truncates the sample; count == 0: zeros
 *     rows 1 .. kept_b - 1   the widened packed rows 0 .. kept_b - 2
 *     rows kept_b .. R - 1   zeros
 *   out_spatials [batch, R, 5], out_mask [batch, R] int64 and the optional out_iou [batch, R, 1] (ref_box and out_iou both
 *   NULL = not written): as the fp32 builder writes them, by its kernel.
 * Every element of every output is written; the caller never clears them.
 *
 * Errors: NULL args, a NULL feat / boxes / offsets / image_wh / out_feat / out_spatials / out_mask, batch < 0, total_rows < 0,
 * max_regions <= 0, feat_dim <= 0, iou_floor negative or NaN, exactly one of ref_box / out_iou NULL, out_kind outside {0, 1}:
 * VB_E_BADARG; feat_dim % 8 != 0, feat or out_feat not 16-byte aligned: VB_E_ALIGN; 2 * total_rows * feat_dim or
 * 4 * batch * max_regions * feat_dim (a byte offset) beyond int64: VB_E_RANGE. batch == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct vbw_task_batch {
    int32_t batch, max_regions, feat_dim, out_kind;
    float iou_floor;                /* 0 = no floor */
    int64_t total_rows;             /* N: rows of feat and boxes */
    const uint16_t* feat;           /* [N, feat_dim] binary16 detector region features, no global row */
    const float* boxes;             /* [N, 4] x1, y1, x2, y2 in pixels */
    const int64_t* offsets;         /* [batch + 1] */
    const int32_t* image_wh;        /* [batch, 2] width, height */
    const int32_t* mean_rows;       /* [batch] or NULL */
    const float* ref_box;           /* [batch, 4] or NULL */
    void* out_feat;                 /* [batch, max_regions, feat_dim] fp32 or bf16 */
    float* out_spatials;            /* [batch, max_regions, 5] */
    int64_t* out_mask;              /* [batch, max_regions] */
    float* out_iou;                 /* [batch, max_regions, 1] or NULL */
} vbw_task_batch;                   /* 112 bytes */

int vbw_task_finish_batch(void* stream, const vbw_task_batch* args);

/* ------------------------------------------------------------------------------------------
 * y[i] = widen(x[i]) for i < n, one launch: 16-byte loads and stores over the first 8 * (n / 8) elements, the last n % 8 one
 * by one - for arrays whose rows are no 16-byte multiples (the [B, R, 1601] region targets). Nothing beyond y[n - 1] is
 * written.
 * Errors: NULL x / y, n < 0: VB_E_BADARG; x or y not 16-byte aligned: VB_E_ALIGN; 4 * n (a byte offset) beyond int64:
 * VB_E_RANGE. n == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
int vbw_widen_f16(void* stream, int64_t n, const uint16_t* x, float* y);

#ifdef __cplusplus
}
#endif
#endif
