/* vilbert_hip_pretrain.h - the NCE masked-region loss of pre-training (visual_target == 2) in libvilbert_hip.so.
 *
 * The export lists of the other headers are pinned name by name by their tests, so these entry points live here under the
 * prefix `vbp_`. Same conventions as the other headers: C linkage, device pointers, `stream` is a hipStream_t passed as
 * void*, every call only enqueues work on it (no allocation, no synchronisation, graph-capture safe), return 0 = ok,
 * > 0 = hipError_t from the launch, < 0 = VB_E_* argument error, checked before anything is launched. rows == 0 launches
 * nothing, writes nothing and returns 0. No floating-point atomics: every result is bit-identical from run to run. The
 * ctypes mirror is vilbert/_native.py: PRETRAIN_SIGNATURES (checked against this text by tests/test_nce_index.py).
 *
 * The loss (reference vilbert.py:1523-1575): a labelled region's predicted feature predict[r, :] is scored against its own
 * target feature and against n_neg = n_across + n_inside other rows of the flat target table [batch * regions, dim]
 * (regions: without the global row), and the loss is the cross entropy of those 1 + n_neg scores with class 0. The
 * [rows, 1 + n_neg, dim] tensor of candidate features the reference builds is never materialised. */
#ifndef VILBERT_HIP_PRETRAIN_H
#define VILBERT_HIP_PRETRAIN_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * neg_idx[r, j] = the table row of negative j of labelled region region_idx[r] (= b * regions + r'), the function of
 * csrc/nce_index.h under `seed`: j < n_across a region of another sample, the others another region of the same sample.
 * One launch. A device step counter registered with vb_set_seed_epoch is mixed into the seed exactly as vb_dropout does, so
 * a replayed graph draws fresh negatives. An entry of region_idx outside [0, batch * regions) gives a row of -1.
 * VB_E_BADARG: a NULL pointer, rows < 0, batch < 1, regions < 1, a negative count, n_across + n_inside < 1, batch < 2 with
 * n_across > 0, regions < 2 with n_inside > 0. VB_E_RANGE: batch * regions or rows * n_neg beyond int64 / 2.
 * ------------------------------------------------------------------------------------------ */
int vbp_nce_negatives(void* stream, int64_t rows, const int64_t* region_idx, int32_t batch, int32_t regions, int32_t n_across,
                      int32_t n_inside, uint64_t seed, int64_t* neg_idx);

/* floats of vbp_nce_fwd's workspace: one partial sum per block of its first launch (never more than 4096); 0 for rows <= 0 */
int64_t vbp_nce_workspace(int64_t rows);

/* ------------------------------------------------------------------------------------------
 * Per row r with valid[r] != 0 (valid: one byte per row, NULL = every row):
 *     score[0] = <table[pos_idx[r]], predict[r]>,  score[1 + j] = <table[neg_idx[r, j]], predict[r]>
 *     row_loss = logsumexp(score) - score[0]
 * loss[0] = sum(row_loss) / count[0]; `count` is a DEVICE scalar (the number of valid rows as float - the host need not
 * know it); 0 / 0 gives NaN like torch's mean over no rows. The sum has a fixed order: each block of the first launch stores
 * one partial into `workspace` (vbp_nce_workspace(rows) floats), a one-block second launch adds them in index order.
 * Invalid rows contribute 0; neither their index entries nor the table rows these name are read.
 * dsave (optional, NULL = forward only; row stride lds >= dim): the UNSCALED gradient
 *     dsave[r, :] = sum_c (softmax(score)_c - [c == 0]) * table[cand_c, :],  zeros for invalid rows
 * computed in the same pass, while the candidate rows are still cache-resident; vbp_nce_bwd then is one scale.
 * Rows are read with 16-byte loads when predict, table (and dsave) are 16-byte aligned and the row strides are multiples
 * of 4; any dim >= 1 and any alignment is served. An index outside [0, table_rows) makes that row's loss (and dsave) NaN
 * instead of being followed. Row strides: ldp, ldt (, lds) >= dim, elements between dim and the stride are not touched.
 * VB_E_BADARG: a NULL required pointer, rows < 0, dim < 1, n_neg < 1, table_rows < 1, a stride < dim.
 * VB_E_RANGE: n_neg > 4095, rows * stride, rows * n_neg or table_rows * ldt beyond int64.
 * ------------------------------------------------------------------------------------------ */
int vbp_nce_fwd(void* stream, int64_t rows, int32_t dim, int32_t n_neg, const float* predict, int64_t ldp, const float* table,
                int64_t table_rows, int64_t ldt, const int64_t* pos_idx, const int64_t* neg_idx, const uint8_t* valid,
                const float* count, float* workspace, float* loss, float* dsave, int64_t lds);

/* dpredict[r, :] = grad_loss[0] / count[0] * dsave[r, :] for valid rows, exact zeros for invalid ones (whatever the scale);
 * grad_loss and count are device scalars. One launch. The target table gets no gradient. Row strides lds, ldd >= dim;
 * elements between dim and ldd are not touched. Errors as above. */
int vbp_nce_bwd(void* stream, int64_t rows, int32_t dim, const float* dsave, int64_t lds, const uint8_t* valid,
                const float* grad_loss, const float* count, float* dpredict, int64_t ldd);

#ifdef __cplusplus
}
#endif
#endif
