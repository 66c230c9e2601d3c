// Host-side validation of the optional row map of an output + feed-forward block (vb_ffn_block.row_map; layers.hip, rowmap.hip).
// Plain C++ for the host compiler too (no HIP header): tests/row_map_driver.cpp evaluates it under the host sanitizers.
#pragma once
#include <stdint.h>

#include "gemm_plan.h"   // the C ABI header, vb_aligned16

namespace vbrows {

// Layout of vb_ffn_block.full_ws (floats; R = src_rows) of a mapped block's backward that ran its reductions over rows at full
// size on zero-expanded operands. Every [R, .] array starts on a 16-byte boundary (H, I multiples of 4); the per-row words
// come last. The backward now reduces over the compact rows and uses the FIRST R words of full_ws only (the inverse map): the
// size of full_ws is not validated, so a caller may pass R words, or a buffer of this layout as before.
struct FullWs {
    long dy, sum2, sum1, a1, h, d_sum2, d_sum2_drop, d_pre, d_a1, d_sum1_drop, stats, inv, total;
    FullWs(long R, long H, long I) {
        long o = 0;
        auto take = [&o](long n) { const long at = o; o += n; return at; };
        dy = take(R * H); sum2 = take(R * H); sum1 = take(R * H); a1 = take(R * H); h = take(R * I);
        d_sum2 = take(R * H); d_sum2_drop = take(R * H); d_pre = take(R * I); d_a1 = take(R * H); d_sum1_drop = take(R * H);
        stats = take(4 * R);      // mean1, rstd1, mean2, rstd2
        inv = take(R);            // int32: compact row of every full row, or -1
        total = o;                // = R (8 H + 2 I + 5)
    }
};

// 0, or the error code of a block whose map cannot be served: fp32 only, 16-byte rows, row counts the int32 map and the
// kernels' index arithmetic can hold. The map's VALUES live on the device: the kernels treat every entry outside
// [0, src_rows) as a padding row.
inline int check_row_map(const vb_ffn_block& f, bool b16, bool backward) {
    if (f.row_map == nullptr) return 0;
    if (b16 || f.ctx_rows == nullptr || f.M <= 0 || f.M > INT32_MAX || f.src_rows <= 0 || f.src_rows > INT32_MAX || f.H <= 0 ||
        f.Hc <= 0 || f.I <= 0)
        return VB_E_BADARG;
    if (f.H % 4 != 0 || f.Hc % 4 != 0 || f.I % 4 != 0) return VB_E_ALIGN;
    if (!vb_aligned16(f.ctx) || !vb_aligned16(f.x) || !vb_aligned16(f.ctx_rows) || !vb_aligned16(f.sum1) || !vb_aligned16(f.a1) ||
        !vb_aligned16(f.sum2) || !vb_aligned16(f.h))
        return VB_E_ALIGN;
    if (backward) {
        if (f.d_ctx_full == nullptr || f.d_sum1_full == nullptr || f.full_ws == nullptr) return VB_E_BADARG;
        if (!vb_aligned16(f.d_ctx_full) || !vb_aligned16(f.d_sum1_full) || !vb_aligned16(f.full_ws) || !vb_aligned16(f.dy) ||
            !vb_aligned16(f.d_ctx) || !vb_aligned16(f.d_sum2) || !vb_aligned16(f.d_sum2_drop) || !vb_aligned16(f.d_sum1_drop) ||
            !vb_aligned16(f.d_pre) || !vb_aligned16(f.d_a1))
            return VB_E_ALIGN;
    }
    return 0;
}

}  // namespace vbrows
