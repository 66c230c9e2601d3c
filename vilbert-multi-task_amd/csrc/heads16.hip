// Row kernels of the pre-training poolers, heads and losses on the bf16 stream (include/vilbert_hip_heads.h, prefix vbh_):
//   gather / invert / scatter   rowmap.hip's row kernels on bf16 rows: the rows the heads read, out of and back into
//                               the [B * T, H] encoder output, 16 bytes per access, row strides allowed
//   ragged weight shadow        fp32 w [n, K] -> bf16 w16 [n_pad, K] and wt16 [K, n_pad], n_pad = 256 ceil(n / 256), pad exact
//                               zeros (the tied 30,522-wide MLM decoder, the 1,601-wide region decoder), + the padded bias
//   loss backwards              cross entropy: G [rows, n_pad] and its transpose GT [n_pad, m_pad] in bf16 from ONE pass
//                               over the fp32 logits (the transpose through LDS, both outputs leave as 16-byte stores);
//                               KL: the row-major form
//   pooler ReLU backward        bf16(dy * (y > 0))
//   GELU backward of a head     bf16(dy * gelu'), gelu' = the act_grad the forward GEMM saved (both bf16)
// No atomics, nothing allocated; the loss gradients are the functions loss.hip calls (row_kit.h), rounded once.
#include "common.h"
#include "row_kit.h"

#include "../../include/vilbert_hip_heads.h"

namespace {

constexpr int H_THREADS = 256;
constexpr int H_TILE = KIT_TILE;           // rows and columns of a transposing tile (row_kit.h)
constexpr long H_MAX_N = 1L << 21;         // widths / row counts whose 64-wide tiles still fit a grid dimension
constexpr long H_MAX_BLOCKS = 4096;        // grid-stride kernels

// grid (K / 64, n_pad / 64)
__global__ __launch_bounds__(H_THREADS) void shadow_ragged_kernel(int n, int K, const float* __restrict__ w, long ldw,
                                                                  const float* __restrict__ bias,
                                                                  unsigned short* __restrict__ w16,
                                                                  unsigned short* __restrict__ wt16, long n_pad,
                                                                  float* __restrict__ bias_pad) {
    __shared__ unsigned tile[H_TILE][33];
    const TileXY t;
    const int r0 = blockIdx.y * H_TILE, c0 = blockIdx.x * H_TILE;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = t.tr + 32 * i, r = r0 + row;
        v4i v = {0, 0, 0, 0};
        if (r < n) {
            float f[8];
            load8(w + (long)r * ldw + c0 + t.tc, f);
            v = pack8(f);
        }
        if (w16 != nullptr) *reinterpret_cast<v4i*>(w16 + (long)r * K + c0 + t.tc) = v;
        tile_put(tile, row, t.tc, v);
    }
    if (blockIdx.x == 0 && bias_pad != nullptr && threadIdx.x < H_TILE) {
        const int r = r0 + threadIdx.x;
        bias_pad[r] = (bias != nullptr && r < n) ? bias[r] : 0.f;
    }
    if (wt16 == nullptr) return;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int col = t.tr + 32 * i;
        *reinterpret_cast<v4i*>(wt16 + (long)(c0 + col) * n_pad + r0 + t.tc) = tile_get_t(tile, col, t.tc);
    }
}

// The cross-entropy gradient as the producer of tile_rows16_kernel (row_kit.h): G, its transpose GT and the column sums from
// ONE pass over the fp32 logits. Rows with the ignore label and columns beyond n are zeros.
struct XentGradRows {
    static constexpr bool TRANSPOSE = true;
    const float* logits; long ld; int vec;
    const int64_t* labels; int64_t ignore;
    const float *lse, *gout, *count;
    __device__ float scale() const { return gout[0] / count[0]; }
    __device__ bool operator()(long r, int c, int n, float g, float (&f)[8]) const {
        const int64_t lab = labels[r];
        if (lab == ignore || c >= n) return false;
        const float l = lse[r];
        load8(logits + r * ld + c, c, n, vec, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = c + e < n ? xent_grad(f[e], l, c + e == lab, g) : 0.f;
        return true;
    }
};

__global__ __launch_bounds__(H_THREADS) void kl_bwd16_kernel(long rows, int n, int chunks, const float* __restrict__ scores,
                                                             long ld, const float* __restrict__ target, long ldt, int vec,
                                                             const float* __restrict__ lse, const float* __restrict__ tsum,
                                                             const float* __restrict__ gout, float divisor,
                                                             const float* __restrict__ divisor_dev,
                                                             unsigned short* __restrict__ G, long ldg) {
    const float g = gout[0] / (divisor_dev != nullptr ? divisor_dev[0] : divisor);
    const long total = rows * chunks;
    for (long i = (long)blockIdx.x * H_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * H_THREADS) {
        const long r = i / chunks;
        const int c = (int)(i - r * chunks) * 8;
        v4i v = {0, 0, 0, 0};
        if (c < n) {
            const float* x = scores + r * ld + c;
            const float* tg = target + r * ldt + c;
            const float l = lse[r], ts = tsum[r];
            float f[8], q[8];
            load8(x, c, n, vec, f);
            load8(tg, c, n, vec, q);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = c + e < n ? kl_grad(f[e], l, ts, q[e], g) : 0.f;
            v = pack8(f);
        }
        *reinterpret_cast<v4i*>(G + r * ldg + c) = v;
    }
}

__global__ __launch_bounds__(H_THREADS) void relu_bwd16_kernel(long rows, int cols8, const float* __restrict__ dy, long ldd,
                                                               const float* __restrict__ y, long ldy,
                                                               unsigned short* __restrict__ out, long ldo) {
    const long total = rows * cols8;
    for (long i = (long)blockIdx.x * H_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * H_THREADS) {
        const long r = i / cols8, c = (i - r * cols8) * 8;
        float f[8], a[8];
        load8(dy + r * ldd + c, f);
        load8(y + r * ldy + c, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] *= a[e] > 0.f ? 1.f : 0.f;      // a product, not a select: dy * 0 keeps its sign (and Inf * 0 its NaN)
        *reinterpret_cast<v4i*>(out + r * ldo + c) = pack8(f);
    }
}

__global__ __launch_bounds__(H_THREADS) void mul16_kernel(long rows, int cols8, const unsigned short* __restrict__ a, long lda,
                                                          const unsigned short* __restrict__ b, long ldb,
                                                          unsigned short* __restrict__ out, long ldo) {
    const long total = rows * cols8;
    for (long i = (long)blockIdx.x * H_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * H_THREADS) {
        const long r = i / cols8, c = (i - r * cols8) * 8;
        const v4i x = *reinterpret_cast<const v4i*>(a + r * lda + c), y = *reinterpret_cast<const v4i*>(b + r * ldb + c);
        float f[8], q[8];
        bf16_unpack8(x, f);
        bf16_unpack8(y, q);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] *= q[e];
        *reinterpret_cast<v4i*>(out + r * ldo + c) = pack8(f);
    }
}

}  // namespace

extern "C" int64_t vbh_padded(int64_t n) { return vb_padded256(n); }

extern "C" int vbh_gather_rows_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* src, int64_t lds, int64_t src_rows,
                                    const int32_t* map, uint16_t* out, int64_t ldo) {
    if (rows < 0 || src_rows < 1 || cols < 1 || lds < cols || ldo < cols) return VB_E_BADARG;
    if (!src || !map || !out) return VB_E_BADARG;
    if (cols % 8 != 0 || !vb_row16_ok(src, lds) || !vb_row16_ok(out, ldo)) return VB_E_ALIGN;
    if (!vb_extent_ok(rows, ldo) || !vb_extent_ok(src_rows, lds)) return VB_E_RANGE;
    if (rows == 0) return 0;
    return vbrows::move_rows((hipStream_t)stream, (long)rows, cols / 8, src, (long)(lds / 8), (long)src_rows, map, out,
                             (long)(ldo / 8), H_MAX_BLOCKS);
}

extern "C" int vbh_invert_map(void* stream, int64_t full_rows, int64_t rows, const int32_t* map, int32_t* inv) {
    if (rows < 0 || full_rows < 0 || !inv || (!map && rows > 0)) return VB_E_BADARG;
    if (rows > INT32_MAX || full_rows > INT32_MAX) return VB_E_RANGE;
    if (full_rows == 0) return 0;
    return vbrows::invert((hipStream_t)stream, (long)full_rows, (long)rows, map, inv);
}

extern "C" int vbh_scatter_rows_bf16(void* stream, int64_t full_rows, int32_t cols, const uint16_t* compact, int64_t ldc,
                                     int64_t rows, const int32_t* inv, uint16_t* full, int64_t ldf) {
    if (rows < 0 || full_rows < 0 || cols < 1 || ldc < cols || ldf < cols) return VB_E_BADARG;
    if ((!compact && rows > 0) || !inv || !full) return VB_E_BADARG;
    if (cols % 8 != 0 || !vb_row16_ok(compact, ldc) || !vb_row16_ok(full, ldf)) return VB_E_ALIGN;
    if (!vb_extent_ok(rows, ldc) || !vb_extent_ok(full_rows, ldf)) return VB_E_RANGE;
    if (full_rows == 0) return 0;
    return vbrows::move_rows((hipStream_t)stream, (long)full_rows, cols / 8, compact, (long)(ldc / 8), (long)rows, inv, full,
                             (long)(ldf / 8), H_MAX_BLOCKS);
}

extern "C" int vbh_weight_shadow_ragged(void* stream, int32_t n, int32_t K, const float* w, int64_t ldw, const float* bias,
                                        uint16_t* w16, uint16_t* wt16, float* bias_pad) {
    if (!w || (!w16 && !wt16) || n < 1 || K < 1 || ldw < K) return VB_E_BADARG;
    if (K % 64 != 0 || !vb_row32_ok(w, ldw) || !vb_aligned16(w16) || !vb_aligned16(wt16)) return VB_E_ALIGN;
    if (n > H_MAX_N) return VB_E_RANGE;
    const long n_pad = vb_padded256(n);
    hipLaunchKernelGGL(shadow_ragged_kernel, dim3((unsigned)(K / H_TILE), (unsigned)(n_pad / H_TILE)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (int)n, (int)K, w, (long)ldw, bias, w16, wt16, n_pad, bias_pad);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_xent_bwd_bf16(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const int64_t* labels,
                                 int64_t ignore_index, const float* lse, const float* grad_loss, const float* count,
                                 uint16_t* G, int64_t ldg, uint16_t* GT, int64_t ldgt, float* colsum_part) {
    const long n_pad = vb_padded256(n), m_pad = vb_padded256(rows);
    if (rows < 0 || n < 1 || ld < n || ldg < n_pad || (GT != nullptr && ldgt < m_pad)) return VB_E_BADARG;
    if (!logits || !labels || !lse || !grad_loss || !count || !G) return VB_E_BADARG;
    if (!vb_row16_ok(G, ldg) || (GT != nullptr && !vb_row16_ok(GT, ldgt))) return VB_E_ALIGN;
    if (rows > H_MAX_N || n > H_MAX_N || !vb_extent_ok(rows, ld) || !vb_extent_ok(rows, ldg) ||
        (GT != nullptr && !vb_extent_ok(n_pad, ldgt)))
        return VB_E_RANGE;
    if (rows == 0) return 0;
    const long row_tiles = GT != nullptr ? m_pad / H_TILE : (rows + H_TILE - 1) / H_TILE;
    const XentGradRows prod{logits, (long)ld, vb_row32_ok(logits, ld) ? 1 : 0, labels, ignore_index, lse, grad_loss, count};
    hipLaunchKernelGGL(tile_rows16_kernel<XentGradRows>, dim3((unsigned)row_tiles, (unsigned)(n_pad / H_TILE)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (long)rows, (int)n, prod, G, (long)ldg, GT, (long)ldgt, colsum_part, n_pad);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vbh_colsum_parts_count(int64_t rows) { return rows <= 0 ? 0 : (rows + H_TILE - 1) / H_TILE; }

extern "C" int vbh_colsum_parts(void* stream, int64_t parts, int32_t n, const float* part, int64_t ldp, float* out) {
    if (parts < 0 || n < 1 || ldp < n || !part || !out) return VB_E_BADARG;
    if (!vb_extent_ok(parts, ldp)) return VB_E_RANGE;
    if (parts == 0) return 0;
    return vbrows::colsum_finish((hipStream_t)stream, (long)parts, (int)n, part, (long)ldp, out);
}

extern "C" int vbh_kl_bwd_bf16(void* stream, int64_t rows, int32_t n, const float* scores, int64_t ld, const float* target,
                               int64_t ldt, const float* lse, const float* tsum, const float* grad_loss, float divisor,
                               const float* divisor_dev, uint16_t* G, int64_t ldg) {
    const long n_pad = vb_padded256(n);
    if (rows < 0 || n < 1 || ld < n || ldt < n || ldg < n_pad) return VB_E_BADARG;
    if (!scores || !target || !lse || !tsum || !grad_loss || !G) return VB_E_BADARG;
    if (!vb_row16_ok(G, ldg)) return VB_E_ALIGN;
    if (n > H_MAX_N || !vb_extent_ok(rows, ld) || !vb_extent_ok(rows, ldt) || !vb_extent_ok(rows, ldg)) return VB_E_RANGE;
    if (rows == 0) return 0;
    const int chunks = (int)(n_pad / 8);
    hipLaunchKernelGGL(kl_bwd16_kernel, dim3(vb_grid_for(rows * chunks, H_THREADS, H_MAX_BLOCKS)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (long)rows, (int)n, chunks, scores, (long)ld, target, (long)ldt,
                       vb_row32_ok(scores, ld) && vb_row32_ok(target, ldt) ? 1 : 0, lse, tsum, grad_loss, divisor, divisor_dev, G,
                       (long)ldg);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_relu_bwd_bf16(void* stream, int64_t rows, int32_t cols, const float* dy, int64_t ldd, const float* y,
                                 int64_t ldy, uint16_t* out, int64_t ldo) {
    if (rows < 0 || cols < 1 || ldd < cols || ldy < cols || ldo < cols) return VB_E_BADARG;
    if (!dy || !y || !out) return VB_E_BADARG;
    if (cols % 8 != 0 || !vb_row32_ok(dy, ldd) || !vb_row32_ok(y, ldy) || !vb_row16_ok(out, ldo)) return VB_E_ALIGN;
    if (!vb_extent_ok(rows, ldd) || !vb_extent_ok(rows, ldy) || !vb_extent_ok(rows, ldo)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(relu_bwd16_kernel, dim3(vb_grid_for(rows * (cols / 8), H_THREADS, H_MAX_BLOCKS)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (long)rows, cols / 8, dy, (long)ldd, y, (long)ldy, out, (long)ldo);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_mul_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* a, int64_t lda, const uint16_t* b,
                            int64_t ldb, uint16_t* out, int64_t ldo) {
    if (rows < 0 || cols < 1 || lda < cols || ldb < cols || ldo < cols) return VB_E_BADARG;
    if (!a || !b || !out) return VB_E_BADARG;
    if (cols % 8 != 0 || !vb_row16_ok(a, lda) || !vb_row16_ok(b, ldb) || !vb_row16_ok(out, ldo)) return VB_E_ALIGN;
    if (!vb_extent_ok(rows, lda) || !vb_extent_ok(rows, ldb) || !vb_extent_ok(rows, ldo)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(mul16_kernel, dim3(vb_grid_for(rows * (cols / 8), H_THREADS, H_MAX_BLOCKS)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (long)rows, cols / 8, a, (long)lda, b, (long)ldb, out, (long)ldo);
    VB_LAUNCH_CHECK();
    return 0;
}
