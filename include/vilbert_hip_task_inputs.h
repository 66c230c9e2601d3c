/* vilbert_hip_task_inputs.h - device-side building of a fine-tuning batch in libvilbert_hip.so: a source hands over PACKED
 * region data (the regions of all samples back to back, pixel boxes, image sizes, sparse answers or a reference box) and the
 * device writes the padded model inputs and the two target kinds of the task list that the reference's datasets build per sample
 * in numpy (vilbert/datasets/_image_features_reader.py:144-176, vqa_dataset.py:275-310, refer_expression_dataset.py:19-56 and
 * 241-296).
 *
 * The export lists of the other headers are pinned name by name by their tests, so this side lives here under the prefix
 * `vbd_`. Same conventions as those headers: C linkage, device pointers, `stream` is a hipStream_t passed as void*, every call
 * only enqueues work on it (no allocation, no synchronisation, no atomics, graph-capture safe), return 0 = ok, > 0 = hipError_t
 * from the launch, < 0 = VB_E_* argument error, checked before anything is launched. The ctypes mirror is vilbert/_native.py:
 * TASK_INPUT_SIGNATURES / TaskBatchArgs (checked against this text by tests/test_task_batch.py); the arithmetic below is
 * restated in numpy by tests/task_batch_restatement.py, and the kernels are held to it bit for bit
 * (tests/test_task_batch_gpu.py). Every fp32 operation below is a single IEEE operation rounded to nearest: nothing is
 * contracted into a fused multiply-add. */
#ifndef VILBERT_HIP_TASK_INPUTS_H
#define VILBERT_HIP_TASK_INPUTS_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Padded inputs of one batch from packed regions. Sample b owns the packed rows offsets[b] .. offsets[b + 1] - 1 (n_b rows);
 * R = max_regions, kept_b = min(n_b + 1, R). The words of `offsets` and `mean_rows` live on the device and are clamped before
 * any address is formed (csrc/task_rows.h): start = clamp(offsets[b], 0, total_rows), n_b = clamp(offsets[b + 1] - start, 0,
 * total_rows - start), mean_rows[b] to [0, n_b]. Every element of every output is written; the caller never clears them.
 *
 *   out_feat [batch, R, feat_dim]
 *     row 0                  the fp32 sum of the first count = mean_rows[b] (NULL: n_b) packed rows IN ROW ORDER, divided in fp32
 *                            by (float)count - over all count rows, also where R truncates the sample; count == 0: zeros
 *     rows 1 .. kept_b - 1   packed rows 0 .. kept_b - 2
 *     rows kept_b .. R - 1   zeros
 *   out_spatials [batch, R, 5], with w = (float)W, h = (float)H, wh = (float)((int64_t)W * H) of image_wh[b] = {W, H}
 *     row 0                  0, 0, 1, 1, 1
 *     kept row r >= 1        x1 / w, y1 / h, x2 / w, y2 / h, ((y2 - y1) * (x2 - x1)) / wh     of packed box r - 1
 *     padding rows           zeros
 *   out_mask [batch, R] int64: 1 for r < kept_b, else 0
 *   out_iou [batch, R, 1] (optional: ref_box and out_iou both NULL = not written), the reference's iou() with its + 1 pixel
 *   convention of the row's pixel box a (row 0: 0, 0, W, H as floats) against g = ref_box[b]:
 *       iw = (min(a.x2, g.x2) - max(a.x1, g.x1)) + 1, below 0: 0; ih likewise in y
 *       area(q) = ((q.x2 - q.x1) + 1) * ((q.y2 - q.y1) + 1)
 *       v = (iw * ih) / ((area(a) + area(g)) - iw * ih);  v < iou_floor: 0 (iou_floor == 0 switches the floor off)
 *     padding rows: 0.
 *
 * Errors: NULL args, a NULL feat / boxes / offsets / image_wh / out_feat / out_spatials / out_mask, batch < 0, total_rows < 0,
 * max_regions <= 0, feat_dim <= 0, iou_floor negative or NaN, exactly one of ref_box / out_iou NULL: VB_E_BADARG;
 * feat_dim % 4 != 0, feat or out_feat not 16-byte aligned: VB_E_ALIGN; 4 * total_rows * feat_dim or
 * 4 * batch * max_regions * feat_dim (a byte offset) beyond int64: VB_E_RANGE. batch == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct vbd_task_batch {
    int32_t batch, max_regions, feat_dim;
    float iou_floor;                /* 0 = no floor; the refer-expression training split uses 0.5 */
    int64_t total_rows;             /* N: rows of feat and boxes */
    const float* feat;              /* [N, feat_dim] detector region features, no global row */
    const float* boxes;             /* [N, 4] x1, y1, x2, y2 in pixels */
    const int64_t* offsets;         /* [batch + 1] */
    const int32_t* image_wh;        /* [batch, 2] width, height */
    const int32_t* mean_rows;       /* [batch] or NULL: leading rows of a sample that enter its mean */
    const float* ref_box;           /* [batch, 4] or NULL */
    float* out_feat;                /* [batch, max_regions, feat_dim] */
    float* out_spatials;            /* [batch, max_regions, 5] */
    int64_t* out_mask;              /* [batch, max_regions] */
    float* out_iou;                 /* [batch, max_regions, 1] or NULL */
} vbd_task_batch;                   /* 104 bytes */

int vbd_task_finish_batch(void* stream, const vbd_task_batch* args);

/* ------------------------------------------------------------------------------------------
 * Dense soft-label target from sparse answers, one launch: target[r, c] for c in [0, num_labels) is scores[r, k] of the LAST k
 * in [0, K) with labels[r, k] == c, or 0 where there is none (torch's scatter_ on a CPU tensor, applied in order). labels are
 * padded with -1; a label outside [0, num_labels) is ignored. target has row stride ldt elements; the elements between
 * num_labels and ldt are never touched. Every element in range is written exactly once: no clearing, no race.
 * Errors: NULL labels / scores / target, rows < 0, num_labels <= 0, K <= 0, ldt < num_labels: VB_E_BADARG; 4 * rows * ldt or
 * 4 * rows * K (a byte offset) beyond int64: VB_E_RANGE. rows == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
int vbd_dense_target(void* stream, int64_t rows, int32_t num_labels, int32_t K, const int32_t* labels, const float* scores,
                     float* target, int64_t ldt);

#ifdef __cplusplus
}
#endif
#endif
