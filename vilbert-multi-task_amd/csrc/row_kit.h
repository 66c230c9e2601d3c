// Device toolkit of the row kernels (heads16.hip, finetune16.hip, bf16_helpers.hip, rowmap.hip, loss.hip, task_loss.hip, nce.hip,
// rowops.h): each piece written once -
//   the bf16 pair format       a 32-bit word holds two bf16 values, the lower column in the low half; unpacking is exact, the
//                              rounding of a store is bf16_round.h's
//   8 fp32 values of a row     with a guarded tail
//   block reduction            of a fixed association (the loss values are compared bit for bit)
//   64 x 64 bf16 tile          transposed through LDS, and the per-64-rows column sums that ride on the same thread map
//   loss gradients             cross entropy and KL from the saved log-sum-exp: one expression for the fp32 and the bf16 kernels
#pragma once
#include "common.h"

typedef int v4i __attribute__((ext_vector_type(4)));

// ---- bf16 pairs --------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// four consecutive bf16 values (8 bytes) as fp32
__device__ __forceinline__ f32x4 bf16_unpack4(uint2 w) { return f32x4{bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y)}; }

// the 8 bf16 values of a 16-byte chunk as fp32
__device__ __forceinline__ void bf16_unpack8(v4i v, float* f) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[2 * k] = bf16_lo((unsigned)v[k]);
        f[2 * k + 1] = bf16_hi((unsigned)v[k]);
    }
}

// 8 fp32 values rounded into a 16-byte chunk
__device__ __forceinline__ v4i pack8(const float* v) {
    return v4i{(int)vb_bf16_pack(v[0], v[1]), (int)vb_bf16_pack(v[2], v[3]), (int)vb_bf16_pack(v[4], v[5]),
               (int)vb_bf16_pack(v[6], v[7])};
}

// f = 8 consecutive fp32 values at a 16-byte aligned x: two 16-byte loads
__device__ __forceinline__ void load8(const float* __restrict__ x, float (&f)[8]) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x), b = *reinterpret_cast<const f32x4*>(x + 4);
    f[0] = a[0]; f[1] = a[1]; f[2] = a[2]; f[3] = a[3]; f[4] = b[0]; f[5] = b[1]; f[6] = b[2]; f[7] = b[3];
}

// f = the columns c .. c + 7 of a row of n columns, x pointing at column c; zeros beyond n. The two 16-byte loads when the row
// is 16-byte addressable (vec) and all 8 columns are inside the row, scalar loads otherwise.
__device__ __forceinline__ void load8(const float* __restrict__ x, int c, int n, bool vec, float (&f)[8]) {
    if (vec && c + 8 <= n) {
        load8(x, f);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = c + e < n ? x[e] : 0.f;
    }
}

// ---- block reduction ---------------------------------------------------------------------------------------------
// Sum or maximum over a block of THREADS threads, every thread gets the result: butterfly over the 64 lanes of a wave, one
// word of `scratch` per wave, then scratch[0] op scratch[1] op ... in that order.
template <bool MAX, int THREADS>
__device__ __forceinline__ float block_reduce(float v, float* scratch) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float o = __shfl_xor(v, off, 64);
        v = MAX ? fmaxf(v, o) : v + o;
    }
    __syncthreads();                       // scratch may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = scratch[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) r = MAX ? fmaxf(r, scratch[w]) : r + scratch[w];
    return r;
}

// ---- 64 x 64 tiles of 256 threads --------------------------------------------------------------------------------
constexpr int KIT_TILE = 64;               // rows and columns of a tile

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

// Column sums of a tile's 64 rows: thread t (TileXY) hands in cs = the sums of its 8 columns over its two rows, and after the
// caller's __syncthreads() thread t < 64 adds the 32 thread rows of column t in order - the same bits on every run.
__device__ __forceinline__ void tile_colsum_put(float (*colred)[KIT_TILE + 1], const TileXY& t, const float (&cs)[8]) {
#pragma unroll
    for (int e = 0; e < 8; ++e) colred[t.tr][t.tc + e] = cs[e];
}
__device__ __forceinline__ float tile_colsum_get(float (*colred)[KIT_TILE + 1]) {
    float a = 0.f;
#pragma unroll 8
    for (int k = 0; k < 32; ++k) a += colred[k][threadIdx.x];
    return a;
}

// fp32 values -> bf16 rows G [rows, ldg] padded with zero columns to n_pad, optionally their transpose GT [n_pad, ldgt] and
// optionally, per 64 rows, the fp32 column sums of the UNROUNDED values (colsum_part [row tiles, n_pad]): one pass, every output
// leaves as 16-byte stores. Grid (row tiles, n_pad / 64); with GT the row tiles cover ldgt's padded rows, else the rows.
// P produces the values (a compile-time choice, passed by value):
//   float P::scale() const                                              read once per thread, handed back as g
//   bool P::operator()(long r, int c, int n, float g, float (&f)[8])    the columns c .. c + 7 of row r < rows (zeros beyond
//                                                                       n); false: the whole chunk is zeros
//   P::TRANSPOSE                                                        whether GT may be asked for (else no tile in LDS)
template <class P>
__global__ __launch_bounds__(256) void tile_rows16_kernel(long rows, int n, const P prod, unsigned short* __restrict__ G, long ldg,
                                                          unsigned short* __restrict__ GT, long ldgt,
                                                          float* __restrict__ colsum_part, long n_pad) {
    __shared__ unsigned tile[P::TRANSPOSE ? KIT_TILE : 1][33];
    __shared__ float colred[32][KIT_TILE + 1];
    const TileXY t;
    const long r0 = (long)blockIdx.x * KIT_TILE;
    const int c0 = blockIdx.y * KIT_TILE, c = c0 + t.tc;
    const float g = prod.scale();
    float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // fp32 column sums of this thread's two rows, before the rounding
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = t.tr + 32 * i;
        const long r = r0 + row;
        v4i v = {0, 0, 0, 0};
        if (r < rows) {
            float f[8];
            if (prod(r, c, n, g, f)) {
                v = pack8(f);
#pragma unroll
                for (int e = 0; e < 8; ++e) cs[e] += f[e];
            }
            *reinterpret_cast<v4i*>(G + r * ldg + c) = v;
        }
        if (P::TRANSPOSE) tile_put(tile, row, t.tc, v);
    }
    const bool sums = colsum_part != nullptr && r0 < rows;      // block-uniform
    const bool transpose = P::TRANSPOSE && GT != nullptr;
    if (sums) tile_colsum_put(colred, t, cs);
    if (!transpose && !sums) return;
    __syncthreads();
    if (sums && threadIdx.x < KIT_TILE) colsum_part[(long)blockIdx.x * n_pad + c0 + threadIdx.x] = tile_colsum_get(colred);
    if (!transpose) return;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int col = t.tr + 32 * i;
        *reinterpret_cast<v4i*>(GT + (long)(c0 + col) * ldgt + r0 + t.tc) = tile_get_t(tile, col, t.tc);
    }
}

// ---- loss gradients ----------------------------------------------------------------------------------------------
// d loss / d logit of the mean cross entropy: (softmax - onehot) * g, softmax = exp(x - lse)
__device__ __forceinline__ float xent_grad(float x, float lse, bool is_label, float g) {
    return (expf(x - lse) - (is_label ? 1.f : 0.f)) * g;
}
// d/dx_j of -sum_k t_k (x_k - lse) = softmax_j * sum(t) - t_j
__device__ __forceinline__ float kl_grad(float x, float lse, float tsum, float t, float g) {
    return (expf(x - lse) * tsum - t) * g;
}
