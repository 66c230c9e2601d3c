// Row kernels of the pre-training poolers, heads and losses on the bf16 stream (include/vilbert_hip_heads.h, prefix vbh_):
//   gather / invert / scatter   the bf16 twins of rowmap.hip's row kernels: the rows the heads read, out of and back into
//                               the [B * T, H] encoder output, 16 bytes per access, row strides allowed
//   ragged weight shadow        fp32 w [n, K] -> bf16 w16 [n_pad, K] and wt16 [K, n_pad], n_pad = 256 ceil(n / 256), pad exact
//                               zeros (the tied 30,522-wide MLM decoder, the 1,601-wide region decoder), + the padded bias
//   loss backwards              cross entropy: G [rows, n_pad] and its transpose GT [n_pad, m_pad] in bf16 from ONE pass
//                               over the fp32 logits (the transpose through LDS, both outputs leave as 16-byte stores);
//                               KL: the row-major form
//   pooler ReLU backward        bf16(dy * (y > 0))
//   GELU backward of a head     bf16(dy * gelu'), gelu' = the act_grad the forward GEMM saved (both bf16)
// No atomics, nothing allocated; the expressions of the loss gradients are those of loss.hip, rounded once.
#include "common.h"

#include "../../include/vilbert_hip_heads.h"

namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int H_THREADS = 256;
constexpr int H_TILE = 64;                 // rows and columns of a transposing tile
constexpr long H_MAX_N = 1L << 21;         // widths / row counts whose 64-wide tiles still fit a grid dimension
constexpr long H_MAX_BLOCKS = 4096;        // grid-stride kernels

inline long padded(long n) { return n <= 0 ? 0 : (n + 255) / 256 * 256; }
// a * b must stay inside int64 (the kernels index with it)
inline bool extent_ok(int64_t a, int64_t b) { return a <= 0 || b <= INT64_MAX / a; }
inline bool row16_ok(const void* p, int64_t ld) { return vb_aligned16(p) && ld % 8 == 0; }
inline bool row32_ok(const void* p, int64_t ld) { return vb_aligned16(p) && ld % 4 == 0; }

inline unsigned grid_for(long items) {
    long blocks = (items + H_THREADS - 1) / H_THREADS;
    if (blocks > H_MAX_BLOCKS) blocks = H_MAX_BLOCKS;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

__device__ __forceinline__ v4i pack8(const float* v) {
    return v4i{(int)vb_bf16_pack(v[0], v[1]), (int)vb_bf16_pack(v[2], v[3]), (int)vb_bf16_pack(v[4], v[5]),
               (int)vb_bf16_pack(v[6], v[7])};
}

// out[r] = src[map[r]], +0 for a map entry outside the source
__global__ __launch_bounds__(H_THREADS) void gather_rows16_kernel(long rows, int cols8, const unsigned short* __restrict__ src,
                                                                  long lds, long src_rows, const int32_t* __restrict__ map,
                                                                  unsigned short* __restrict__ out, long ldo) {
    const long n = rows * cols8;
    for (long i = (long)blockIdx.x * H_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * H_THREADS) {
        const long r = i / cols8, c = (i - r * cols8) * 8;
        const long s = map[r];
        v4i v = {0, 0, 0, 0};
        if (s >= 0 && s < src_rows) v = *reinterpret_cast<const v4i*>(src + s * lds + c);
        *reinterpret_cast<v4i*>(out + r * ldo + c) = v;
    }
}

// full[R] = compact[inv[R]], +0 where no compact row stands for R: every element written once
__global__ __launch_bounds__(H_THREADS) void scatter_rows16_kernel(long full_rows, int cols8,
                                                                   const unsigned short* __restrict__ compact, long ldc,
                                                                   long rows, const int32_t* __restrict__ inv,
                                                                   unsigned short* __restrict__ full, long ldf) {
    const long n = full_rows * cols8;
    for (long i = (long)blockIdx.x * H_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * H_THREADS) {
        const long R = i / cols8, c = (i - R * cols8) * 8;
        const long r = inv[R];
        v4i v = {0, 0, 0, 0};
        if (r >= 0 && r < rows) v = *reinterpret_cast<const v4i*>(compact + r * ldc + c);
        *reinterpret_cast<v4i*>(full + R * ldf + c) = v;
    }
}

// A 64 x 64 bf16 tile in LDS, two values per word, rows padded to 33 words. Thread t owns the 8 columns tc .. tc + 7 of
// the rows tr and tr + 32 on the way in, and the 8 ROWS tc .. tc + 7 of the columns tr and tr + 32 on the way out.
struct TileXY {
    int tr, tc;
    __device__ TileXY() : tr(threadIdx.x >> 3), tc((threadIdx.x & 7) * 8) {}
};

__device__ __forceinline__ void tile_put(unsigned (*tile)[33], int row, int tc, v4i v) {
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[row][(tc >> 1) + k] = (unsigned)v[k];
}

// the 8 values tile[tc .. tc + 7][col], packed as they lie in a row of the transpose
__device__ __forceinline__ v4i tile_get_t(unsigned (*tile)[33], int col, int tc) {
    const int w = col >> 1, sh = (col & 1) * 16;
    v4i o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned lo = (tile[tc + 2 * k][w] >> sh) & 0xffffu, hi = (tile[tc + 2 * k + 1][w] >> sh) & 0xffffu;
        o[k] = (int)(lo | (hi << 16));
    }
    return o;
}

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
            const float* p = w + (long)r * ldw + c0 + t.tc;
            const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
            const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
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

// grid (row tiles, n_pad / 64); with GT the row tiles cover m_pad, without it the rows
__global__ __launch_bounds__(H_THREADS) void xent_bwd16_kernel(long rows, int n, const float* __restrict__ logits, long ld,
                                                               int vec, const int64_t* __restrict__ labels, int64_t ignore,
                                                               const float* __restrict__ lse, const float* __restrict__ gout,
                                                               const float* __restrict__ count,
                                                               unsigned short* __restrict__ G, long ldg,
                                                               unsigned short* __restrict__ GT, long ldgt,
                                                               float* __restrict__ colsum_part, long n_pad) {
    __shared__ unsigned tile[H_TILE][33];
    __shared__ float colred[32][H_TILE + 1];
    const TileXY t;
    const long r0 = (long)blockIdx.x * H_TILE;
    const int c0 = blockIdx.y * H_TILE, c = c0 + t.tc;
    const float g = gout[0] / count[0];
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // fp32 column sums of this thread's two rows, before the rounding
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = t.tr + 32 * i;
        const long r = r0 + row;
        v4i v = {0, 0, 0, 0};
        if (r < rows) {
            const int64_t lab = labels[r];
            if (lab != ignore && c < n) {
                const float* x = logits + r * ld + c;
                const float l = lse[r];
                float f[8];
                if (vec && c + 8 <= n) {
                    const f32x4 a = *reinterpret_cast<const f32x4*>(x), b = *reinterpret_cast<const f32x4*>(x + 4);
                    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) f[e] = c + e < n ? x[e] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < 8; ++e)      // (the expression of loss.hip's xent_bwd_kernel)
                    f[e] = c + e < n ? (expf(f[e] - l) - (c + e == lab ? 1.f : 0.f)) * g : 0.f;
                v = pack8(f);
#pragma unroll
                for (int e = 0; e < 8; ++e) cs[e] += f[e];
            }
            *reinterpret_cast<v4i*>(G + r * ldg + c) = v;
        }
        tile_put(tile, row, t.tc, v);
    }
    const bool sums = colsum_part != nullptr && r0 < rows;      // block-uniform
    if (sums) {
#pragma unroll
        for (int e = 0; e < 8; ++e) colred[t.tr][t.tc + e] = cs[e];
    }
    if (GT == nullptr && !sums) return;
    __syncthreads();
    if (sums && threadIdx.x < H_TILE) {                          // rows in a fixed order: the same bits on every run
        float a = 0.f;
#pragma unroll 8
        for (int k = 0; k < 32; ++k) a += colred[k][threadIdx.x];
        colsum_part[(long)blockIdx.x * n_pad + c0 + threadIdx.x] = a;
    }
    if (GT == nullptr) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int col = t.tr + 32 * i;
        *reinterpret_cast<v4i*>(GT + (long)(c0 + col) * ldgt + r0 + t.tc) = tile_get_t(tile, col, t.tc);
    }
}

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
            if (vec && c + 8 <= n) {
                const f32x4 a = *reinterpret_cast<const f32x4*>(x), b = *reinterpret_cast<const f32x4*>(x + 4);
                const f32x4 ta = *reinterpret_cast<const f32x4*>(tg), tb = *reinterpret_cast<const f32x4*>(tg + 4);
                f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
                q[0] = ta[0]; q[1] = ta[1]; q[2] = ta[2]; q[3] = ta[3]; q[4] = tb[0]; q[5] = tb[1]; q[6] = tb[2]; q[7] = tb[3];
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    f[e] = c + e < n ? x[e] : 0.f;
                    q[e] = c + e < n ? tg[e] : 0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e)          // (the expression of loss.hip's kl_bwd_kernel)
                f[e] = c + e < n ? (expf(f[e] - l) * ts - q[e]) * g : 0.f;
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
        const float* d = dy + r * ldd + c;
        const float* a = y + r * ldy + c;
        const f32x4 d0 = *reinterpret_cast<const f32x4*>(d), d1 = *reinterpret_cast<const f32x4*>(d + 4);
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + 4);
        float f[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {            // a product, not a select: dy * 0 keeps its sign (and Inf * 0 its NaN)
            f[e] = d0[e] * (a0[e] > 0.f ? 1.f : 0.f);
            f[4 + e] = d1[e] * (a1[e] > 0.f ? 1.f : 0.f);
        }
        *reinterpret_cast<v4i*>(out + r * ldo + c) = pack8(f);
    }
}

// out[j] += part[0][j] + part[1][j] + ... in that order, j < n
__global__ __launch_bounds__(H_THREADS) void colsum_parts_kernel(long parts, int n, const float* __restrict__ part, long ldp,
                                                                 float* __restrict__ out) {
    const int j = blockIdx.x * H_THREADS + threadIdx.x;
    if (j >= n) return;
    float a = 0.f;
    for (long p = 0; p < parts; ++p) a += part[p * ldp + j];
    out[j] += a;
}

__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

__global__ __launch_bounds__(H_THREADS) void mul16_kernel(long rows, int cols8, const unsigned short* __restrict__ a, long lda,
                                                          const unsigned short* __restrict__ b, long ldb,
                                                          unsigned short* __restrict__ out, long ldo) {
    const long total = rows * cols8;
    for (long i = (long)blockIdx.x * H_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * H_THREADS) {
        const long r = i / cols8, c = (i - r * cols8) * 8;
        const v4i x = *reinterpret_cast<const v4i*>(a + r * lda + c), y = *reinterpret_cast<const v4i*>(b + r * ldb + c);
        v4i o;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            o[k] = (int)vb_bf16_pack(bf16_lo((unsigned)x[k]) * bf16_lo((unsigned)y[k]), bf16_hi((unsigned)x[k]) * bf16_hi((unsigned)y[k]));
        *reinterpret_cast<v4i*>(out + r * ldo + c) = o;
    }
}

}  // namespace

extern "C" int64_t vbh_padded(int64_t n) { return padded(n); }

extern "C" int vbh_gather_rows_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* src, int64_t lds, int64_t src_rows,
                                    const int32_t* map, uint16_t* out, int64_t ldo) {
    if (rows < 0 || src_rows < 1 || cols < 1 || lds < cols || ldo < cols) return VB_E_BADARG;
    if (!src || !map || !out) return VB_E_BADARG;
    if (cols % 8 != 0 || !row16_ok(src, lds) || !row16_ok(out, ldo)) return VB_E_ALIGN;
    if (!extent_ok(rows, ldo) || !extent_ok(src_rows, lds)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(gather_rows16_kernel, dim3(grid_for(rows * (cols / 8))), dim3(H_THREADS), 0, (hipStream_t)stream,
                       (long)rows, cols / 8, src, (long)lds, (long)src_rows, map, out, (long)ldo);
    VB_LAUNCH_CHECK();
    return 0;
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
    if (cols % 8 != 0 || !row16_ok(compact, ldc) || !row16_ok(full, ldf)) return VB_E_ALIGN;
    if (!extent_ok(rows, ldc) || !extent_ok(full_rows, ldf)) return VB_E_RANGE;
    if (full_rows == 0) return 0;
    hipLaunchKernelGGL(scatter_rows16_kernel, dim3(grid_for(full_rows * (cols / 8))), dim3(H_THREADS), 0, (hipStream_t)stream,
                       (long)full_rows, cols / 8, compact, (long)ldc, (long)rows, inv, full, (long)ldf);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_weight_shadow_ragged(void* stream, int32_t n, int32_t K, const float* w, int64_t ldw, const float* bias,
                                        uint16_t* w16, uint16_t* wt16, float* bias_pad) {
    if (!w || (!w16 && !wt16) || n < 1 || K < 1 || ldw < K) return VB_E_BADARG;
    if (K % 64 != 0 || !row32_ok(w, ldw) || !vb_aligned16(w16) || !vb_aligned16(wt16)) return VB_E_ALIGN;
    if (n > H_MAX_N) return VB_E_RANGE;
    const long n_pad = padded(n);
    hipLaunchKernelGGL(shadow_ragged_kernel, dim3((unsigned)(K / H_TILE), (unsigned)(n_pad / H_TILE)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (int)n, (int)K, w, (long)ldw, bias, w16, wt16, n_pad, bias_pad);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_xent_bwd_bf16(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const int64_t* labels,
                                 int64_t ignore_index, const float* lse, const float* grad_loss, const float* count,
                                 uint16_t* G, int64_t ldg, uint16_t* GT, int64_t ldgt, float* colsum_part) {
    const long n_pad = padded(n), m_pad = padded(rows);
    if (rows < 0 || n < 1 || ld < n || ldg < n_pad || (GT != nullptr && ldgt < m_pad)) return VB_E_BADARG;
    if (!logits || !labels || !lse || !grad_loss || !count || !G) return VB_E_BADARG;
    if (!row16_ok(G, ldg) || (GT != nullptr && !row16_ok(GT, ldgt))) return VB_E_ALIGN;
    if (rows > H_MAX_N || n > H_MAX_N || !extent_ok(rows, ld) || !extent_ok(rows, ldg) ||
        (GT != nullptr && !extent_ok(n_pad, ldgt)))
        return VB_E_RANGE;
    if (rows == 0) return 0;
    const long row_tiles = GT != nullptr ? m_pad / H_TILE : (rows + H_TILE - 1) / H_TILE;
    hipLaunchKernelGGL(xent_bwd16_kernel, dim3((unsigned)row_tiles, (unsigned)(n_pad / H_TILE)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (long)rows, (int)n, logits, (long)ld, row32_ok(logits, ld) ? 1 : 0, labels,
                       ignore_index, lse, grad_loss, count, G, (long)ldg, GT, (long)ldgt, colsum_part, n_pad);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vbh_colsum_parts_count(int64_t rows) { return rows <= 0 ? 0 : (rows + H_TILE - 1) / H_TILE; }

extern "C" int vbh_colsum_parts(void* stream, int64_t parts, int32_t n, const float* part, int64_t ldp, float* out) {
    if (parts < 0 || n < 1 || ldp < n || !part || !out) return VB_E_BADARG;
    if (!extent_ok(parts, ldp)) return VB_E_RANGE;
    if (parts == 0) return 0;
    hipLaunchKernelGGL(colsum_parts_kernel, dim3((unsigned)((n + H_THREADS - 1) / H_THREADS)), dim3(H_THREADS), 0,
                       (hipStream_t)stream, (long)parts, (int)n, part, (long)ldp, out);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_kl_bwd_bf16(void* stream, int64_t rows, int32_t n, const float* scores, int64_t ld, const float* target,
                               int64_t ldt, const float* lse, const float* tsum, const float* grad_loss, float divisor,
                               const float* divisor_dev, uint16_t* G, int64_t ldg) {
    const long n_pad = padded(n);
    if (rows < 0 || n < 1 || ld < n || ldt < n || ldg < n_pad) return VB_E_BADARG;
    if (!scores || !target || !lse || !tsum || !grad_loss || !G) return VB_E_BADARG;
    if (!row16_ok(G, ldg)) return VB_E_ALIGN;
    if (n > H_MAX_N || !extent_ok(rows, ld) || !extent_ok(rows, ldt) || !extent_ok(rows, ldg)) return VB_E_RANGE;
    if (rows == 0) return 0;
    const int chunks = (int)(n_pad / 8);
    hipLaunchKernelGGL(kl_bwd16_kernel, dim3(grid_for(rows * chunks)), dim3(H_THREADS), 0, (hipStream_t)stream, (long)rows,
                       (int)n, chunks, scores, (long)ld, target, (long)ldt, row32_ok(scores, ld) && row32_ok(target, ldt) ? 1 : 0,
                       lse, tsum, grad_loss, divisor, divisor_dev, G, (long)ldg);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_relu_bwd_bf16(void* stream, int64_t rows, int32_t cols, const float* dy, int64_t ldd, const float* y,
                                 int64_t ldy, uint16_t* out, int64_t ldo) {
    if (rows < 0 || cols < 1 || ldd < cols || ldy < cols || ldo < cols) return VB_E_BADARG;
    if (!dy || !y || !out) return VB_E_BADARG;
    if (cols % 8 != 0 || !row32_ok(dy, ldd) || !row32_ok(y, ldy) || !row16_ok(out, ldo)) return VB_E_ALIGN;
    if (!extent_ok(rows, ldd) || !extent_ok(rows, ldy) || !extent_ok(rows, ldo)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(relu_bwd16_kernel, dim3(grid_for(rows * (cols / 8))), dim3(H_THREADS), 0, (hipStream_t)stream, (long)rows,
                       cols / 8, dy, (long)ldd, y, (long)ldy, out, (long)ldo);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbh_mul_bf16(void* stream, int64_t rows, int32_t cols, const uint16_t* a, int64_t lda, const uint16_t* b,
                            int64_t ldb, uint16_t* out, int64_t ldo) {
    if (rows < 0 || cols < 1 || lda < cols || ldb < cols || ldo < cols) return VB_E_BADARG;
    if (!a || !b || !out) return VB_E_BADARG;
    if (cols % 8 != 0 || !row16_ok(a, lda) || !row16_ok(b, ldb) || !row16_ok(out, ldo)) return VB_E_ALIGN;
    if (!extent_ok(rows, lda) || !extent_ok(rows, ldb) || !extent_ok(rows, ldo)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(mul16_kernel, dim3(grid_for(rows * (cols / 8))), dim3(H_THREADS), 0, (hipStream_t)stream, (long)rows,
                       cols / 8, a, (long)lda, b, (long)ldb, out, (long)ldo);
    VB_LAUNCH_CHECK();
    return 0;
}
