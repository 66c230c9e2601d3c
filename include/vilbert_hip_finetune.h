/* vilbert_hip_finetune.h - the skinny-output linear of the fine-tuning heads on the bf16 stream in libvilbert_hip.so
 * (csrc/finetune16.hip): a linear with 1 .. 4 outputs (`vision_logit`, `linguisic_logit` of VILBertForVLTasks: one output per
 * token / region row) read straight off the bf16 hidden states, its input dropout fused - the dropped input is never written.
 * Last in the file: the cast of a decoder's fp32 logit gradient that also leaves its fp32 column sums (vbf_cast_rows_colsum).
 *
 * The export lists of the other headers are pinned name by name by their tests, so these entry points live here under the
 * prefix `vbf_`. Same conventions as vilbert_hip_heads.h: C linkage, device pointers, `stream` is a hipStream_t passed as
 * void*, every call only enqueues work on it (no allocation, no synchronisation, graph-capture safe), return 0 = ok,
 * > 0 = hipError_t from the launch, < 0 = VB_E_* argument error, checked before anything is launched. rows == 0 launches
 * nothing, writes nothing and returns 0. No floating-point atomics: every result is bit-identical from run to run. The
 * ctypes mirror is vilbert/_native.py: FINETUNE_SIGNATURES (checked against this text by tests/test_finetune16_abi.py).
 *
 * Shapes: n = the output width, 1 <= n <= VBF_MAX_N; K = the input width, K % 8 == 0, 8 <= K <= VBF_MAX_K (a wave holds a
 * whole row of the n weight rows in registers); x bf16 [rows, K] (uint16_t bit patterns, row stride ldx >= K, in ELEMENTS);
 * w the fp32 MASTER weight [n, K] (row stride ldw >= K) - no bf16 shadow: at this width the weight lives in registers.
 * Dropout: drop(x[r, k]) = keep(seed', r * K + k, p) ? x[r, k] * scale : 0 with csrc/rng.h's mask, the element index that of
 * the DENSE [rows, K] tensor whatever ldx is (vb_dropout's convention), seed' = the seed with the registered device step
 * counter mixed in (vb_set_seed_epoch), scale = fp32 1 / (1 - p). p == 0 draws nothing and ignores the seed.
 * Errors of every entry point: VB_E_BADARG - a NULL required pointer, rows < 0, n outside 1 .. VBF_MAX_N, K < 8, a stride
 * below its width, p outside [0, 1). VB_E_ALIGN - K % 8, ldx % 8 (lddx % 8), ldw % 4 (lddw % 4), a bf16 or fp32 pointer not
 * 16-byte aligned. VB_E_RANGE - K beyond VBF_MAX_K, rows beyond int32, a rows-times-stride product beyond int64. */
#ifndef VILBERT_HIP_FINETUNE_H
#define VILBERT_HIP_FINETUNE_H

#include "vilbert_hip.h"

#define VBF_MAX_N 4
#define VBF_MAX_K 2048

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * out[r, j] = sum_k drop(x[r, k]) * w[j, k] + bias[j] + row_add[r]      (products and sums fp32)
 * out fp32 [rows, n], row stride ldo >= n (any; elements between n and ldo are not touched). bias fp32 [n] or NULL; row_add
 * fp32 [rows] or NULL, added to every column (the additive region mask of `vision_logit`). Every row of x is read once, 16
 * bytes per lane and load; one wave per row, the sum over a row is a cross-lane reduction in a fixed order. One launch.
 * ------------------------------------------------------------------------------------------ */
int vbf_skinny_linear_fwd(void* stream, int64_t rows, int32_t K, int32_t n, const uint16_t* x, int64_t ldx, const float* w,
                          int64_t ldw, const float* bias, const float* row_add, float* out, int64_t ldo, float p,
                          uint64_t seed);

/* ------------------------------------------------------------------------------------------
 * dx[r, k] = bf16(keep(r, k) * scale * sum_j dy[r, j] * w[j, k])        (the fp32 value rounded once, csrc/bf16_round.h)
 * dy fp32 [rows, n] (row stride ldy >= n), dx bf16 [rows, K] (row stride lddx >= K): every element of
 * dx[:, 0 .. K) is written exactly once - +0 where the mask drops -, elements between K and lddx are not touched. One launch.
 * ------------------------------------------------------------------------------------------ */
int vbf_skinny_linear_bwd_input(void* stream, int64_t rows, int32_t K, int32_t n, const float* dy, int64_t ldy, const float* w,
                                int64_t ldw, uint16_t* dx, int64_t lddx, float p, uint64_t seed);

/* floats of the workspace vbf_skinny_linear_bwd_weight needs for (rows, K, n): parts * (n * K + 4) with parts =
 * min(ceil(rows / 32), 512) row ranges; 0 for rows <= 0 or a (K, n) the kernels do not serve */
int64_t vbf_skinny_wgrad_workspace(int64_t rows, int32_t K, int32_t n);

/* ------------------------------------------------------------------------------------------
 * dw[j, k] += sum_r dy[r, j] * drop(x[r, k])        db[j] += sum_r dy[r, j]        (db may be NULL)
 * Both are ADDED into their fp32 destinations (gradient-arena slices; dw [n, K] with row stride lddw >= K, db [n]), as
 * vbh_colsum_parts does. Two launches through the workspace (fp32, 16-byte aligned, at least
 * vbf_skinny_wgrad_workspace(rows, K, n) floats): one wave per range of consecutive rows sums its rows in row order into
 * registers and writes one partial row; the second launch adds the partial rows up in a fixed order. The same bits on
 * every run. VB_E_BADARG also for a NULL workspace.
 * ------------------------------------------------------------------------------------------ */
int vbf_skinny_linear_bwd_weight(void* stream, int64_t rows, int32_t K, int32_t n, const float* dy, int64_t ldy,
                                 const uint16_t* x, int64_t ldx, float* dw, int64_t lddw, float* db, float* workspace, float p,
                                 uint64_t seed);

/* ------------------------------------------------------------------------------------------
 * The fp32 gradient of a decoder's logits as the bf16 operand of the GEMMs in front (vb_cast_rows_f32_bf16) and, from the same
 * read, its column sums in fp32 (the decoder's bias gradient, which must not be summed from rounded values): with n_pad =
 * vbh_padded(n) = 256 ceil(n / 256)
 *     G [rows, n_pad] (row stride ldg >= n_pad)      G[r, j] = bf16(x[r, j]), +0 in columns n .. n_pad
 *     colsum_part [ceil(rows / 64), n_pad]           row p holds, per column, the sum of x over rows 64 p .. 64 p + 63 in a fixed
 *                                                    order (pad columns 0): vbh_colsum_parts over it is the column sum
 * x fp32 [rows, n], row stride ldx >= n. One launch.
 * VB_E_BADARG: a NULL pointer, rows < 0, n < 1, ldx < n, ldg < n_pad. VB_E_ALIGN: ldx % 4, ldg % 8, a pointer not 16-byte
 * aligned. VB_E_RANGE: rows or n beyond 2^21, rows * ldx or rows * ldg beyond int64.
 * ------------------------------------------------------------------------------------------ */
int vbf_cast_rows_colsum(void* stream, int64_t rows, int32_t n, const float* x, int64_t ldx, uint16_t* G, int64_t ldg,
                         float* colsum_part);

#ifdef __cplusplus
}
#endif
#endif
