// Shared pieces of the row kernels (layernorm.hip, embed.hip): one 64-lane wave owns a row, a lane holds 4 consecutive
// columns of every 256-column chunk (chunk i, lane l -> columns (64 i + l) 4 ...), NV = chunks per row. The row stays in
// registers between the statistics passes, so every element crosses HBM once each way. Device and host helpers only.
#pragma once
#include <initializer_list>
#include <type_traits>

#include "common.h"
#include "mx8.h"
#include "row_kit.h"

namespace vbrow {

constexpr int ROWS_PER_BLOCK = 4;  // 4 waves

// first of the 4 columns that lane `lane` holds of chunk i (a macro: through a function the compiler loses what it knows of
// the sign of the column and widens the row-offset multiplies that follow)
#define VB_LANE_COL(i, lane) (((i) * 64 + (lane)) * 4)

// wave_sum of R independent values side by side (R dependent shuffle chains interleaved)
template <int R>
__device__ __forceinline__ void wave_sum_rows(float (&a)[R]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        float t[R];
#pragma unroll
        for (int r = 0; r < R; ++r) t[r] = __shfl_xor(a[r], off, 64);
#pragma unroll
        for (int r = 0; r < R; ++r) a[r] += t[r];
    }
}

// Row I/O of a lane's 4 columns, per element type of the row: `packed` is what a lane loads (*(const packed*)p) and keeps
// resident, unpack() widens it, store() rounds and writes.
struct RowF32 {
    using elem = float;
    using packed = f32x4;
    static constexpr unsigned ALIGN = 16;
    static constexpr bool PREFETCH = false;
    static __device__ __forceinline__ packed zero() { return f32x4{0.f, 0.f, 0.f, 0.f}; }
    static __device__ __forceinline__ f32x4 unpack(const packed w) { return w; }
    static __device__ __forceinline__ void store(elem* p, const f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
};
struct RowBF16 {
    using elem = unsigned short;
    using packed = uint2;
    static constexpr unsigned ALIGN = 8;
    static constexpr bool PREFETCH = true;   // layernorm_bwd_kernel: request the next row before this row's reductions
    static __device__ __forceinline__ packed zero() { return uint2{0u, 0u}; }
    static __device__ __forceinline__ f32x4 unpack(const packed w) { return bf16_unpack4(w); }
    static __device__ __forceinline__ void store(elem* p, const f32x4 v) {
        *reinterpret_cast<uint2*>(p) = uint2{vb_bf16_pack(v[0], v[1]), vb_bf16_pack(v[2], v[3])};
    }
};

// y = gamma * (x - mean) * rstd + beta, TF style (biased variance, eps inside the sqrt), two-pass statistics
// reference vilbert.py:313-317
template <int NV>
__device__ __forceinline__ void ln_finish(f32x4 (&x)[NV], int n_cols, int lane, const float* gamma,
                                          const float* beta, float eps, float* yrow, float* mean_out,
                                          float* rstd_out, float* presum_row = nullptr,
                                          unsigned char* qrow = nullptr, float* qscale = nullptr,
                                          unsigned* mx_words = nullptr, long mx_rows = 0) {
    if (presum_row != nullptr) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            if (col < n_cols) *reinterpret_cast<f32x4*>(presum_row + col) = x[i];
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        if (col < n_cols) s += (x[i][0] + x[i][1]) + (x[i][2] + x[i][3]);
    }
    const float mean = wave_sum(s) / (float)n_cols;
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        if (col < n_cols) {
            x[i] -= mean;
            v += (x[i][0] * x[i][0] + x[i][1] * x[i][1]) + (x[i][2] * x[i][2] + x[i][3] * x[i][3]);
        }
    }
    const float var = wave_sum(v) / (float)n_cols;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (lane == 0) {
        if (mean_out != nullptr) *mean_out = mean;
        if (rstd_out != nullptr) *rstd_out = rstd;
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        if (col < n_cols) {
            const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col);
            const f32x4 b = *reinterpret_cast<const f32x4*>(beta + col);
            x[i] = g * (x[i] * rstd) + b;
            *reinterpret_cast<f32x4*>(yrow + col) = x[i];
            if (qrow != nullptr)
                amax = fmaxf(amax, fmaxf(fmaxf(fabsf(x[i][0]), fabsf(x[i][1])), fmaxf(fabsf(x[i][2]), fabsf(x[i][3]))));
        }
    }
    if (qrow != nullptr && mx_words != nullptr) {
        // MX codes of the row (mx8.h): chunk i = columns 256 i .. 256 i + 255, a 32-column block = 8 consecutive lanes;
        // mx_words = scale plane base + this row, plane stride mx_rows words (bit-identical to vb_quantize_rows_mx on y)
        const int nkt = n_cols >> 7;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            const bool ok = col < n_cols;
            const int kt = 2 * i + (lane >> 5);
            mx_quant_chunk(x[i], ok, lane, kt, nkt, reinterpret_cast<unsigned*>(qrow + (ok ? col : 0)),
                           mx_words + (long)(kt < nkt ? kt : 0) * mx_rows);
        }
    } else if (qrow != nullptr) {
        // the row's e4m3 codes + scale for the fp8 linears that consume it (same recipe, same bits as
        // vb_quantize_rows_fp8 applied to the stored row - csrc/fp8.hip)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        const bool zero = !(amax > 0.f);
        const float inv = zero ? 1.f : 448.0f / amax;
        if (lane == 0) *qscale = zero ? 1.f : amax / 448.0f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            if (col < n_cols) {
                int w = __builtin_amdgcn_cvt_pk_fp8_f32(x[i][0] * inv, x[i][1] * inv, 0, false);
                w = __builtin_amdgcn_cvt_pk_fp8_f32(x[i][2] * inv, x[i][3] * inv, w, true);
                *reinterpret_cast<unsigned*>(qrow + col) = (unsigned)w;
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------
inline int nv_for(int n_cols) { return (n_cols + 255) / 256; }

inline int check_cols(int n_cols) {
    if (n_cols <= 0) return VB_E_BADARG;
    if (n_cols % 4 != 0) return VB_E_ALIGN;
    if (n_cols > VB_MAX_LN_COLS) return VB_E_RANGE;
    return 0;
}

inline bool any_null(std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if (p == nullptr) return true;
    return false;
}

// every pointer a multiple of `align` bytes (a power of two); null - an optional argument left out - passes
inline bool all_aligned(unsigned align, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((reinterpret_cast<uintptr_t>(p) & (align - 1)) != 0) return false;
    return true;
}

// Calls f(std::integral_constant<int, NV>) with the instantiated NV that serves rows of nv chunks: 1, 2, 3, 4 and, up to
// MAX, the next of 8 / 16 / 32 (MAX = 4: the bf16 kernels, rows of at most 1,024 columns).
template <int MAX, typename F>
inline void dispatch_nv(int nv, F&& f) {
    static_assert(MAX == 4 || MAX == 16 || MAX == 32, "instantiated widths");
    if (nv == 1) return f(std::integral_constant<int, 1>{});
    if (nv == 2) return f(std::integral_constant<int, 2>{});
    if (nv == 3) return f(std::integral_constant<int, 3>{});
    if constexpr (MAX > 4) {
        if (nv > 16 && MAX > 16) return f(std::integral_constant<int, MAX>{});
        if (nv > 8) return f(std::integral_constant<int, 16>{});
        if (nv > 4) return f(std::integral_constant<int, 8>{});
    }
    return f(std::integral_constant<int, 4>{});
}

}  // namespace vbrow
