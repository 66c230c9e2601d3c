// Streaming helpers of the bf16 TRAINING path (gemm_bf16.hip holds its GEMMs): the casts between fp32 and bf16 tensors, the
// bf16 shadows (row-major AND transposed) of the fp32 master weights, refreshed once per optimizer step, and the column
// sums of a bf16 matrix (bias gradient). Called directly by tests/test_bf16_helpers_gpu.py.
#include "common.h"
#include "row_kit.h"

namespace {

__global__ __launch_bounds__(256) void cast_f32_bf16_kernel(long n8, const float* __restrict__ x, unsigned short* __restrict__ y,
                                                            long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n8) {
        float f[8];
        load8(x + 8 * i, f);
        *reinterpret_cast<v4i*>(y + 8 * i) = pack8(f);
    } else if (i == n8) {
        for (long e = 8 * n8; e < n; ++e) y[e] = (unsigned short)vb_bf16_round(x[e]);
    }
}

// fp32 [rows][n] (row stride ldx) -> bf16 [rows][ldy], columns n .. ldy - 1 zero-filled: the padded bf16 operand of a weight
// gradient whose output width is not a tile multiple (the 30,522-wide MLM decoder: 30,720 = 120 x 256)
__global__ __launch_bounds__(256) void cast_rows_f32_bf16_kernel(long rows, int n, const float* __restrict__ x, long ldx,
                                                                 unsigned short* __restrict__ y, long ldy) {
    const long chunks = ldy / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * chunks) return;
    const long r = i / chunks;
    const int c = (int)(i % chunks) * 8;
    float f[8];
    load8(x + r * ldx + c, c, n, true, f);
    *reinterpret_cast<v4i*>(y + r * ldy + c) = pack8(f);
}

__global__ __launch_bounds__(256) void cast_bf16_f32_kernel(long n8, const unsigned short* __restrict__ x, float* __restrict__ y,
                                                            long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n8) {
        const v4i w = *reinterpret_cast<const v4i*>(x + 8 * i);
        *reinterpret_cast<f32x4*>(y + 8 * i) = bf16_unpack4(uint2{(unsigned)w[0], (unsigned)w[1]});
        *reinterpret_cast<f32x4*>(y + 8 * i + 4) = bf16_unpack4(uint2{(unsigned)w[2], (unsigned)w[3]});
    } else if (i == n8) {
        for (long e = 8 * n8; e < n; ++e) y[e] = bf16_lo(x[e]);
    }
}

// One 64 x 64 tile at (r0, c0) of an fp32 master weight -> its bf16 shadow rows (w16, row stride ld16; may be null) AND their
// transpose (wt16, row stride ldt; may be null) through LDS. 256 threads: thread t owns 4 columns of the rows t / 16 + 16 i.
__device__ __forceinline__ void shadow_tile(int r0, int c0, const float* __restrict__ w, long ldw,
                                            unsigned short* __restrict__ w16, long ld16, unsigned short* __restrict__ wt16,
                                            long ldt) {
    __shared__ unsigned short tile[64][66];
    const int tr = threadIdx.x >> 4, tc = (threadIdx.x & 15) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = tr + 16 * i;
        const f32x4 v = *reinterpret_cast<const f32x4*>(w + (long)(r0 + row) * ldw + c0 + tc);
        const unsigned lo = vb_bf16_pack(v[0], v[1]), hi = vb_bf16_pack(v[2], v[3]);
        if (w16 != nullptr) *reinterpret_cast<uint2*>(w16 + (long)(r0 + row) * ld16 + c0 + tc) = uint2{lo, hi};
        tile[row][tc] = (unsigned short)lo; tile[row][tc + 1] = (unsigned short)(lo >> 16);
        tile[row][tc + 2] = (unsigned short)hi; tile[row][tc + 3] = (unsigned short)(hi >> 16);
    }
    __syncthreads();
    if (wt16 == nullptr) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = tr + 16 * i;      // row of the transposed tile
        const unsigned lo = (unsigned)tile[tc][col] | ((unsigned)tile[tc + 1][col] << 16);
        const unsigned hi = (unsigned)tile[tc + 2][col] | ((unsigned)tile[tc + 3][col] << 16);
        *reinterpret_cast<uint2*>(wt16 + (long)(c0 + col) * ldt + r0 + tc) = uint2{lo, hi};
    }
}

// fp32 master weight [rows, cols] -> bf16 shadow rows (w16 [rows, ld16]) AND its transpose (wt16 [cols, ldt], written at
// column offset col_off = the row offset of this segment inside a stacked weight); grid (cols / 64, rows / 64)
__global__ __launch_bounds__(256) void weight_shadow_kernel(const float* __restrict__ w, long ldw, unsigned short* __restrict__ w16,
                                                            long ld16, unsigned short* __restrict__ wt16, long ldt) {
    shadow_tile(blockIdx.y * 64, blockIdx.x * 64, w, ldw, w16, ld16, wt16, ldt);
}

// the same for EVERY registered weight in one launch (once per optimizer step): block b finds its segment in the table by
// bisection over the segments' first tile
__global__ __launch_bounds__(256) void weight_shadow_multi_kernel(int n_segs, const vb_shadow_seg* __restrict__ tab) {
    int lo = 0, hi = n_segs - 1;
    const long b = blockIdx.x;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid].tile0 <= b) lo = mid; else hi = mid - 1;
    }
    const vb_shadow_seg sg = tab[lo];
    const int t = (int)(b - sg.tile0), tiles_c = sg.cols >> 6;
    shadow_tile((t / tiles_c) * 64, (t % tiles_c) * 64, sg.w, sg.cols, sg.w16, sg.ld16, sg.wt16, sg.ldt);
}

// column sums of a bf16 [rows, cols] matrix (bias gradient): stage 1 - a block owns 256 columns x one row slab, a thread 4
// columns of every fourth row, waves summed through LDS, one partial row per slab; stage 2 - the slabs in order
// (deterministic). out: ADDED into (the gradient arena semantics of the weight gradients).
constexpr int CS_SLABS = 64;
__global__ __launch_bounds__(256) void colsum16_kernel(long rows, int cols, const unsigned short* __restrict__ x, long ldx,
                                                       float* __restrict__ part) {
    __shared__ f32x4 red[3][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = blockIdx.x * 256 + 4 * lane;
    const long per = (rows + CS_SLABS - 1) / CS_SLABS;
    const long lo = blockIdx.y * per, hi = min(rows, lo + per);
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (col < cols)
        for (long r = lo + wave; r < hi; r += 4) {
            const uint2 w = *reinterpret_cast<const uint2*>(x + r * ldx + col);
            s += bf16_unpack4(w);
        }
    if (wave > 0) red[wave - 1][lane] = s;
    __syncthreads();
    if (wave == 0 && col < cols) {
        s += red[0][lane]; s += red[1][lane]; s += red[2][lane];
        *reinterpret_cast<f32x4*>(part + (long)blockIdx.y * cols + col) = s;
    }
}
// out[j] += part[0][j] + part[1][j] + ... in that order, j < n: stage 2 here, and the per-64-rows partial sums the loss
// backward and the cast of heads16.hip leave behind (vbh_colsum_parts)
__global__ __launch_bounds__(256) void colsum_finish_kernel(long parts, int n, const float* __restrict__ part, long ldp,
                                                            float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    float a = 0.f;
    for (long p = 0; p < parts; ++p) a += part[p * ldp + j];
    out[j] += a;
}

}  // namespace

int vbrows::colsum_finish(hipStream_t st, long parts, int n, const float* part, long ldp, float* out) {
    hipLaunchKernelGGL(colsum_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, parts, n, part, ldp, out);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_cast_f32_bf16(void* stream, int64_t n, const float* x, uint16_t* y) {
    if (x == nullptr || y == nullptr || n <= 0) return VB_E_BADARG;
    if (!vb_aligned16(x) || !vb_aligned16(y)) return VB_E_ALIGN;
    const long n8 = n / 8;
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3((unsigned)((n8 + 1 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       n8, x, y, (long)n);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_cast_rows_f32_bf16(void* stream, int64_t rows, int32_t n, const float* x, int64_t ldx, uint16_t* y, int64_t ldy) {
    if (x == nullptr || y == nullptr || rows <= 0 || n <= 0 || ldx < n || ldy < n) return VB_E_BADARG;
    if (!vb_row32_ok(x, ldx) || !vb_row16_ok(y, ldy)) return VB_E_ALIGN;
    const long work = rows * (ldy / 8);
    hipLaunchKernelGGL(cast_rows_f32_bf16_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       (long)rows, (int)n, x, (long)ldx, y, (long)ldy);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_cast_bf16_f32(void* stream, int64_t n, const uint16_t* x, float* y) {
    if (x == nullptr || y == nullptr || n <= 0) return VB_E_BADARG;
    if (!vb_aligned16(x) || !vb_aligned16(y)) return VB_E_ALIGN;
    const long n8 = n / 8;
    hipLaunchKernelGGL(cast_bf16_f32_kernel, dim3((unsigned)((n8 + 1 + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       n8, x, y, (long)n);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_weight_shadow_bf16(void* stream, int32_t rows, int32_t cols, const float* w, int64_t ldw, uint16_t* w16,
                                     int64_t ld16, uint16_t* wt16, int64_t ldt) {
    if (w == nullptr || (w16 == nullptr && wt16 == nullptr) || rows <= 0 || cols <= 0) return VB_E_BADARG;
    if (rows % 64 != 0 || cols % 64 != 0 || ldw % 4 != 0 || !vb_aligned16(w)) return VB_E_ALIGN;
    if (w16 != nullptr && (ld16 % 4 != 0 || ld16 < cols || (reinterpret_cast<uintptr_t>(w16) & 7u) != 0)) return VB_E_ALIGN;
    if (wt16 != nullptr && (ldt % 4 != 0 || ldt < rows || (reinterpret_cast<uintptr_t>(wt16) & 7u) != 0)) return VB_E_ALIGN;
    hipLaunchKernelGGL(weight_shadow_kernel, dim3(cols / 64, rows / 64), dim3(256), 0, static_cast<hipStream_t>(stream), w,
                       (long)ldw, w16, (long)ld16, wt16, (long)ldt);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_weight_shadow_multi(void* stream, int32_t n_segs, const vb_shadow_seg* table, int64_t total_tiles) {
    if (table == nullptr || n_segs <= 0 || total_tiles <= 0 || total_tiles > 0x7fffffffL) return VB_E_BADARG;
    hipLaunchKernelGGL(weight_shadow_multi_kernel, dim3((unsigned)total_tiles), dim3(256), 0, static_cast<hipStream_t>(stream), n_segs,
                       table);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vb_colsum_bf16_workspace(int32_t cols) { return (int64_t)CS_SLABS * cols; }

extern "C" int vb_colsum_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* x, int64_t ldx, float* out,
                              float* workspace) {
    if (x == nullptr || out == nullptr || workspace == nullptr || rows <= 0 || cols <= 0) return VB_E_BADARG;
    if (cols % 4 != 0 || ldx % 4 != 0 || ldx < cols || (reinterpret_cast<uintptr_t>(x) & 7u) != 0 || !vb_aligned16(workspace))
        return VB_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(colsum16_kernel, dim3((cols + 255) / 256, CS_SLABS), dim3(256), 0, st, (long)rows, cols, x, (long)ldx, workspace);
    VB_LAUNCH_CHECK();
    return vbrows::colsum_finish(st, CS_SLABS, cols, workspace, cols, out);
}
