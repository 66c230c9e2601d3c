// Host-side argument checks and launch arithmetic of the row kernels (heads16.hip, finetune16.hip, bf16_helpers.hip, rowmap.hip,
// elementwise.hip, task_loss.hip, nce.hip, batch.hip, task_batch.hip) as HOST-ONLY code: no HIP header, so tests/test_row_checks_host.py compiles it with
// the host compiler and pins every function.
#pragma once
#include <stdint.h>

#include "gemm_plan.h"   // vb_aligned16

// a * b stays inside int64 (the kernels index with it); a <= 0: nothing is indexed
static inline bool vb_extent_ok(int64_t a, int64_t b) { return a <= 0 || b <= INT64_MAX / a; }
// rows * ld elements of `bytes` bytes each whose BYTE offsets stay inside int64 (the batch-finishing kernels form pointers
// from them)
static inline bool vb_byte_extent_ok(int64_t rows, int64_t ld, int64_t bytes) {
    return vb_extent_ok(rows, ld) && (rows <= 0 || rows * ld <= INT64_MAX / bytes);
}
// rows of bf16 / fp32 elements, stride ld elements, that 16-byte accesses may address at every 8th / 4th column
static inline bool vb_row16_ok(const void* p, int64_t ld) { return vb_aligned16(p) && ld % 8 == 0; }
static inline bool vb_row32_ok(const void* p, int64_t ld) { return vb_aligned16(p) && ld % 4 == 0; }
// 256 * ceil(n / 256): the width of the zero-padded bf16 operand of a ragged linear (vbh_padded)
static inline int64_t vb_padded256(int64_t n) { return n <= 0 ? 0 : (n + 255) / 256 * 256; }
// blocks of a grid-stride launch: one thread per item until `cap` blocks, never fewer than one
static inline unsigned vb_grid_for(int64_t items, int threads, int64_t cap) {
    int64_t blocks = (items + threads - 1) / threads;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}
