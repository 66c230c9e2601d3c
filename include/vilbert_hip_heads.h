/* vilbert_hip_heads.h - row kernels of the pre-training poolers, heads and losses on the bf16 stream in libvilbert_hip.so
 * (csrc/heads16.hip).
 *
 * The export lists of the other headers are pinned name by name by their tests, so these entry points live here under the
 * prefix `vbh_`. Same conventions as vilbert_hip_pretrain.h: C linkage, device pointers, `stream` is a hipStream_t passed as
 * void*, every call only enqueues work on it (no allocation, no synchronisation, graph-capture safe), return 0 = ok,
 * > 0 = hipError_t from the launch, < 0 = VB_E_* argument error, checked before anything is launched. rows == 0 launches
 * nothing, writes nothing and returns 0. No floating-point atomics: every result is bit-identical from run to run. The
 * ctypes mirror is vilbert/_native.py: HEADS_SIGNATURES (checked against this text by tests/test_heads16_abi.py).
 *
 * Every bf16 tensor is passed as uint16_t bit patterns; leading dimensions count ELEMENTS; bf16 rows are read and written
 * 16 bytes at a time, so bf16 pointers are 16-byte aligned, bf16 widths and leading dimensions are multiples of 8, fp32
 * pointers are 16-byte aligned and fp32 leading dimensions multiples of 4 (VB_E_ALIGN otherwise) unless stated otherwise.
 * fp32 -> bf16 is the rounding of csrc/bf16_round.h: nearest even, torch's CPU cast bit for bit, a NaN stays a NaN. */
#ifndef VILBERT_HIP_HEADS_H
#define VILBERT_HIP_HEADS_H

#include "vilbert_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 256 * ceil(n / 256): the padded width of a linear whose output width n is not a tile multiple (the tied 30,522-wide MLM
 * decoder: 30,720), and the padded row count m_pad of a transposed gradient; 0 for n <= 0 */
int64_t vbh_padded(int64_t n);

/* ------------------------------------------------------------------------------------------
 * Gather of bf16 rows: out[r, 0 .. cols) = src[map[r], 0 .. cols) for r < rows; an entry of the int32 map outside
 * [0, src_rows) (-1 = padding row) gives a row of +0. Row strides lds, ldo >= cols; elements between cols and ldo are not
 * touched. One launch.
 * VB_E_BADARG: a NULL pointer, rows < 0, src_rows < 1, cols < 1, a stride < cols. VB_E_ALIGN: cols % 8, a stride % 8, src or
 * out not 16-byte aligned. VB_E_RANGE: rows * ldo or src_rows * lds beyond int64.
 * ------------------------------------------------------------------------------------------ */
int vbh_gather_rows_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* src, int64_t lds, int64_t src_rows,
                         const int32_t* map, uint16_t* out, int64_t ldo);

/* inv[R] = the first r < rows with map[r] == R, or -1, for every R < full_rows: each inv[R] is written exactly once, no fill
 * pass in front, no atomics. rows == 0 is served (every inv[R] = -1): the scatter behind it still has to write its zeros.
 * VB_E_BADARG: a NULL pointer (map may be NULL with rows == 0), rows < 0, full_rows < 0. VB_E_RANGE: rows or full_rows
 * beyond int32. full_rows == 0 launches nothing. */
int vbh_invert_map(void* stream, int64_t full_rows, int64_t rows, const int32_t* map, int32_t* inv);

/* ------------------------------------------------------------------------------------------
 * Scatter of bf16 rows: full[R, 0 .. cols) = compact[inv[R], 0 .. cols) for R < full_rows, +0 where inv[R] lies outside
 * [0, rows). Every element of full[:, 0 .. cols) is written exactly once - no fill pass in front, no atomics; elements
 * between cols and ldf are not touched. One launch; full_rows == 0 launches nothing.
 * Errors as for the gather (compact may be NULL with rows == 0).
 * ------------------------------------------------------------------------------------------ */
int vbh_scatter_rows_bf16(void* stream, int64_t full_rows, int32_t cols, const uint16_t* compact, int64_t ldc, int64_t rows,
                          const int32_t* inv, uint16_t* full, int64_t ldf);

/* ------------------------------------------------------------------------------------------
 * Zero-padded bf16 shadow of an fp32 weight w [n, K] (row stride ldw) whose height n is no tile multiple, n_pad =
 * vbh_padded(n):  w16 [n_pad, K] = bf16(w), rows n .. n_pad exact zeros;  wt16 [K, n_pad] = w16^T (columns n .. n_pad
 * zeros);  bias_pad [n_pad] = bias, zero beyond n (bias == NULL: all zeros; bias_pad == NULL: not written). w16 and wt16
 * are dense (row strides K and n_pad); either may be NULL. One launch over 64 x 64 tiles through LDS; rows of w beyond n
 * are never read.
 * VB_E_BADARG: w NULL, w16 and wt16 both NULL, n < 1, K < 1, ldw < K. VB_E_ALIGN: K % 64, ldw % 4, a pointer not 16-byte
 * aligned. VB_E_RANGE: n beyond 2^21.
 * ------------------------------------------------------------------------------------------ */
int vbh_weight_shadow_ragged(void* stream, int32_t n, int32_t K, const float* w, int64_t ldw, const float* bias, uint16_t* w16,
                             uint16_t* wt16, float* bias_pad);

/* ------------------------------------------------------------------------------------------
 * Cross-entropy backward that emits the bf16 operands of the GEMMs behind it (vb_xent_bwd followed by
 * vb_cast_rows_f32_bf16, in one pass over the logits): with n_pad = vbh_padded(n), m_pad = vbh_padded(rows),
 *     G  [rows, n_pad] (row stride ldg >= n_pad)     G[r, j] = bf16((exp(x[r, j] - lse[r]) - [j == labels[r]]) * (grad_loss[0] / count[0]))
 *     GT [n_pad, m_pad] (row stride ldgt >= m_pad)   GT[j, r] = G[r, j]                    (optional: NULL = G only)
 * in the fp32 expression of vb_xent_bwd, rounded once. +0 goes to rows with labels[r] == ignore_index, to columns
 * n .. n_pad of G (rows n .. n_pad of GT) and to columns rows .. m_pad of GT. The transpose goes through LDS (tiles of 64
 * rows x 64 columns); the logits (row stride ld >= n, any alignment: 16-byte loads where ld % 4 == 0 and the pointer is
 * aligned) are read once. grad_loss, count: device scalars. One launch.
 * colsum_part (optional, NULL = none): fp32 [vbh_colsum_parts_count(rows), n_pad] - row p holds, per column, the sum of the
 * UNROUNDED fp32 gradient over rows 64 p .. 64 p + 63 in a fixed order (pad columns 0): the bias gradient of the decoder in
 * front is vbh_colsum_parts over it - fp32 sums of fp32 terms, as vb_xent_bwd + the fp32 weight-gradient kernel gave.
 * VB_E_BADARG: a NULL required pointer, rows < 0, n < 1, ld < n, ldg < n_pad, GT given with ldgt < m_pad.
 * VB_E_ALIGN: ldg % 8, ldgt % 8, G or GT not 16-byte aligned. VB_E_RANGE: rows or n beyond 2^21, rows * ld, rows * ldg or
 * n_pad * ldgt beyond int64.
 * ------------------------------------------------------------------------------------------ */
int vbh_xent_bwd_bf16(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const int64_t* labels,
                      int64_t ignore_index, const float* lse, const float* grad_loss, const float* count, uint16_t* G,
                      int64_t ldg, uint16_t* GT, int64_t ldgt, float* colsum_part);

/* ceil(rows / 64): rows of vbh_xent_bwd_bf16's colsum_part; 0 for rows <= 0 */
int64_t vbh_colsum_parts_count(int64_t rows);

/* out[j] += part[0, j] + part[1, j] + ... + part[parts - 1, j] (in that order: bit-identical from run to run) for j < n; part
 * fp32 [parts, ldp >= n]; out [n] is ADDED into (a gradient-arena slice). One launch; parts == 0 launches nothing.
 * VB_E_BADARG: a NULL pointer, parts < 0, n < 1, ldp < n. VB_E_RANGE: parts * ldp beyond int64. */
int vbh_colsum_parts(void* stream, int64_t parts, int32_t n, const float* part, int64_t ldp, float* out);

/* KL-divergence backward, row-major form only: G [rows, n_pad] = bf16((exp(x - lse[r]) * tsum[r] - target[r, j]) * g),
 * g = grad_loss[0] / (divisor_dev ? divisor_dev[0] : divisor), the fp32 expression of vb_kl_bwd rounded once; +0 in columns
 * n .. n_pad. scores / target: row strides ld, ldt >= n, any alignment. One launch. Errors as above. */
int vbh_kl_bwd_bf16(void* stream, int64_t rows, int32_t n, const float* scores, int64_t ld, const float* target, int64_t ldt,
                    const float* lse, const float* tsum, const float* grad_loss, float divisor, const float* divisor_dev,
                    uint16_t* G, int64_t ldg);

/* ReLU backward of the poolers: out[r, j] = bf16(dy[r, j] * (y[r, j] > 0 ? 1 : 0)) from the fp32 gradient and the fp32
 * OUTPUT of the activation. Row strides ldd, ldy, ldo >= cols. One launch.
 * VB_E_BADARG: a NULL pointer, rows < 0, cols < 1, a stride < cols. VB_E_ALIGN: cols % 8, ldo % 8, ldd % 4, ldy % 4, a
 * pointer not 16-byte aligned. VB_E_RANGE: rows * stride beyond int64. */
int vbh_relu_bwd_bf16(void* stream, int64_t rows, int32_t cols, const float* dy, int64_t ldd, const float* y, int64_t ldy,
                      uint16_t* out, int64_t ldo);

/* GELU backward of a prediction-head transform: out[r, j] = bf16(a[r, j] * b[r, j]), a = the bf16 gradient, b = the bf16
 * act_grad = gelu'(pre-activation) the forward vb_linear_bf16 stored; the fp32 product is rounded once. Row strides lda, ldb,
 * ldo >= cols; out overlaps neither input. One launch. Errors as for vbh_relu_bwd_bf16 (every stride % 8). */
int vbh_mul_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* a, int64_t lda, const uint16_t* b, int64_t ldb,
                 uint16_t* out, int64_t ldo);

#ifdef __cplusplus
}
#endif
#endif
