/* vilbert_hip_store.h - fine-tuning batches from a DEVICE-RESIDENT region store, in libvilbert_hip.so. The detector's regions of
 * a whole dataset (features, pixel boxes, image sizes) are copied to the device once, image after image; a batch is then named
 * by one image index per output sample, and the device gathers each sample's rows itself. A batch costs the bus its indices
 * (and the token arrays), not its feature rows; an image that a task shows several times (the four answers of VCR, the options
 * of retrieval, the pairs of NLVR2) is a repeated index.
 *
 * The call below writes what the packed builders of vilbert_hip_task_inputs.h (fp32 rows) and vilbert_hip_wire.h (binary16
 * rows, fp32 or bf16 feature block) write for a batch whose sample b owns exactly the rows of image image_ids[b] - the same
 * kernels (csrc/feat_rows.h, csrc/task_meta.h) reading their rows through the store's index, to the bit. Those two headers
 * state the per-sample arithmetic; this one states where a sample's rows and per-image words come from.
 *
 * The export lists of the other headers are pinned name by name by their tests, so this side lives here under the prefix
 * `vbr_`. Same conventions as those headers: C linkage, device pointers, `stream` is a hipStream_t passed as void*, the call
 * only enqueues work on it (two launches; no allocation, no synchronisation, no atomics, graph-capture safe), return 0 = ok,
 * > 0 = hipError_t from the launch, < 0 = VB_E_* argument error, checked before anything is launched. The ctypes mirror is
 * vilbert/_native.py: STORE_SIGNATURES / StoreBatchArgs (checked against this text by tests/test_region_store.py); the kernels
 * are held bit for bit to the packed builders (tests/test_region_store_gpu.py). */
#ifndef VILBERT_HIP_STORE_H
#define VILBERT_HIP_STORE_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VBR_FEAT_F32 0
#define VBR_FEAT_F16 1
#define VBR_OUT_F32 0
#define VBR_OUT_BF16 1

/* ------------------------------------------------------------------------------------------
 * Padded inputs of one batch gathered from the store. The store holds num_images images; image i owns the rows
 * image_offsets[i] .. image_offsets[i + 1] - 1 of feat and boxes, has the size image_wh[i] = {W, H} and, with mean_rows, the
 * count mean_rows[i] of leading rows that enter its mean. All of these words, and image_ids, live on the device and cannot be
 * validated by the host. For output sample b, with id = image_ids[b] and R = max_regions:
 *
 *   valid id (0 <= id < num_images): the words of image id are clamped before any address is formed (csrc/store_rows.h,
 *     csrc/task_rows.h): start = clamp(image_offsets[id], 0, total_rows), n = clamp(image_offsets[id + 1] - start, 0,
 *     total_rows - start), mean_rows[id] to [0, n]. Sample b is then what the packed builder writes for a sample that owns the
 *     rows start .. start + n - 1 in an image of size image_wh[id]: row 0 the mean of the leading rows, rows 1 .. kept - 1
 *     (kept = min(n + 1, R)) the rows themselves (widened from binary16 where feat_kind says so, rounded to bf16 where
 *     out_kind says so), zeros after them; the 5-number boxes; mask 1 for r < kept; with ref_box, the IoU of each kept row's
 *     pixel box against ref_box[b], floored by iou_floor. ref_box and every output are indexed by b, never by id: two samples
 *     with the same id may have different reference boxes.
 *   invalid id (negative, >= num_images, any 64-bit pattern): NO store word is read for it - not image_offsets, not image_wh,
 *     not mean_rows - and sample b is all padding: out_feat rows all zero (row 0 too), out_spatials zero, out_mask all 0,
 *     out_iou 0. A mask row without a single 1 is how a caller sees it; a valid id always has out_mask[b, 0] == 1.
 *
 * Every element of every output is written; the caller never clears them. feat_kind / out_kind: VBR_FEAT_F32 with
 * VBR_OUT_F32, VBR_FEAT_F16 with VBR_OUT_F32 or VBR_OUT_BF16 - the three kinds of the packed builders.
 *
 * Errors, in this order: NULL args, batch < 0, total_rows < 0, num_images < 0, max_regions <= 0, feat_dim <= 0, iou_floor
 * negative or NaN, feat_kind or out_kind outside {0, 1}, VBR_OUT_BF16 with VBR_FEAT_F32, a NULL feat / boxes / image_offsets /
 * image_wh / image_ids / out_feat / out_spatials / out_mask, exactly one of ref_box / out_iou NULL: VB_E_BADARG;
 * feat_dim % 4 != 0 (fp32 store) or feat_dim % 8 != 0 (binary16 store), feat or out_feat not 16-byte aligned: VB_E_ALIGN;
 * total_rows * feat_dim * (4 or 2) - a byte offset into the store - or 4 * batch * max_regions * feat_dim beyond int64:
 * VB_E_RANGE. batch == 0 launches nothing and returns 0.
 * ------------------------------------------------------------------------------------------ */
typedef struct vbr_store_batch {
    int32_t batch, max_regions, feat_dim;
    float iou_floor;                /* 0 = no floor */
    int32_t feat_kind, out_kind;
    int64_t total_rows;             /* rows of feat and boxes in the store */
    int64_t num_images;
    const void* feat;               /* [total_rows, feat_dim] fp32 or binary16 */
    const float* boxes;             /* [total_rows, 4] x1, y1, x2, y2 in pixels */
    const int64_t* image_offsets;   /* [num_images + 1] */
    const int32_t* image_wh;        /* [num_images, 2] width, height */
    const int32_t* mean_rows;       /* [num_images] or NULL: all rows of an image enter its mean */
    const int64_t* image_ids;       /* [batch] */
    const float* ref_box;           /* [batch, 4] or NULL */
    void* out_feat;                 /* [batch, max_regions, feat_dim] fp32 or bf16 */
    float* out_spatials;            /* [batch, max_regions, 5] */
    int64_t* out_mask;              /* [batch, max_regions] */
    float* out_iou;                 /* [batch, max_regions, 1] or NULL */
} vbr_store_batch;                  /* 128 bytes */

int vbr_store_finish_batch(void* stream, const vbr_store_batch* args);

#ifdef __cplusplus
}
#endif
#endif
