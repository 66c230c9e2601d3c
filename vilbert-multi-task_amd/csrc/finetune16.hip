// The skinny-output linear of the fine-tuning heads on the bf16 stream (include/vilbert_hip_finetune.h, prefix vbf_):
// out [rows, n] = drop(x) w^T + bias + row_add for n = 1 .. 4 outputs (`vision_logit`, `linguisic_logit`: one logit per region /
// token row) with x the bf16 hidden states and w the fp32 master weight, and its two gradients. Streaming row kernels, bound
// by the one read (or write) of x / dx:
//   forward           one wave per row (grid-stride), the n weight rows in registers (lane l holds the 8 columns of the chunks
//                     l, l + 64, ...: up to VBF_MAX_K / 512 = 4 chunks), 16-byte loads, wave_sum across the lanes
//   input gradient    the same layout; dx = bf16(keep * scale * sum_j dy_j w_j), every chunk stored once
//   weight gradient   stage 1: one wave per range of consecutive rows, dw of that range in registers, one partial row
//                     [n * K + 4] of the workspace per wave (the last 4: the bias gradient); stage 2: the partial rows added
//                     up in a fixed order INTO dw / db
//   cast + column sums   the fp32 gradient of a ragged decoder's logits -> its zero-padded bf16 GEMM operand and, per 64 rows,
//                     fp32 column sums of the unrounded values (the decoder's bias gradient: vbh_colsum_parts adds them up)
// The dropout mask (rng.h) is drawn per element from the index r * K + k of the dense tensor - the dropped input never exists
// in memory. No atomics, nothing allocated.
#include "common.h"
#include "rng.h"
#include "row_kit.h"

#include "../../include/vilbert_hip_finetune.h"

namespace {

constexpr int F_WAVE = 64;
constexpr int F_THREADS = 256;             // forward / input gradient: 4 waves = 4 rows in flight per block
constexpr int F_WAVES = F_THREADS / F_WAVE;
constexpr long F_MAX_BLOCKS = 4096;
constexpr long F_PART_ROWS = 32;           // weight gradient: rows per partial sum ...
constexpr long F_MAX_PARTS = 512;          // ... until this many partial rows, then longer ranges
constexpr int F_RED_COLS = 64;             // stage 2: columns per block, F_THREADS / F_RED_COLS interleaved slices of the parts
constexpr int F_RED_SLICES = F_THREADS / F_RED_COLS;
constexpr int F_TILE = KIT_TILE;           // rows and columns of a tile of the cast with column sums (row_kit.h)
constexpr long F_MAX_TILED = 1L << 21;     // widths / row counts whose 64-wide tiles still fit a grid dimension

inline long parts_for(long rows) {
    const long p = (rows + F_PART_ROWS - 1) / F_PART_ROWS;
    return p > F_MAX_PARTS ? F_MAX_PARTS : p;
}

// lane's chunks of the NN weight rows: w[j][i][e] = w[j, (lane + 64 i) * 8 + e]
template <int NN, int CH>
__device__ __forceinline__ void load_weights(const float* __restrict__ w, long ldw, int K8, int lane, float (&wr)[NN][CH][8]) {
#pragma unroll
    for (int j = 0; j < NN; ++j)
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + F_WAVE * i;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (c < K8) {
                const float* q = w + (long)j * ldw + (long)c * 8;
                a = *reinterpret_cast<const f32x4*>(q);
                b = *reinterpret_cast<const f32x4*>(q + 4);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                wr[j][i][e] = a[e];
                wr[j][i][4 + e] = b[e];
            }
        }
}

// f[e] = drop(f[e]) for the chunk that starts at dense element index i0
__device__ __forceinline__ void drop8(float* f, uint64_t seed, uint64_t i0, float p, float scale) {
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = vb_keep(seed, i0 + (uint64_t)e, p) ? f[e] * scale : 0.f;
}

template <int NN, int CH>
__global__ __launch_bounds__(F_THREADS) void skinny_fwd_kernel(long rows, int K8, const unsigned short* __restrict__ x, long ldx,
                                                               const float* __restrict__ w, long ldw,
                                                               const float* __restrict__ bias,
                                                               const float* __restrict__ row_add, float* __restrict__ out,
                                                               long ldo, float p, float scale, uint64_t seed0,
                                                               const uint64_t* __restrict__ epoch) {
    const int lane = threadIdx.x & (F_WAVE - 1), wave = threadIdx.x >> 6;
    const long K = (long)K8 * 8;
    float wr[NN][CH][8];
    load_weights<NN, CH>(w, ldw, K8, lane, wr);
    const bool drop = p > 0.f;                                   // (uniform)
    const uint64_t seed = drop ? vb_seed_with_epoch(seed0, epoch) : 0;
    for (long r = (long)blockIdx.x * F_WAVES + wave; r < rows; r += (long)gridDim.x * F_WAVES) {
        const unsigned short* xr = x + r * ldx;
        float acc[NN];
#pragma unroll
        for (int j = 0; j < NN; ++j) acc[j] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + F_WAVE * i;
            if (c < K8) {
                float f[8];
                bf16_unpack8(*reinterpret_cast<const v4i*>(xr + (long)c * 8), f);
                if (drop) drop8(f, seed, (uint64_t)(r * K + (long)c * 8), p, scale);
#pragma unroll
                for (int j = 0; j < NN; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[j] = fmaf(f[e], wr[j][i][e], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < NN; ++j) acc[j] = wave_sum(acc[j]);
        if (lane == 0) {
            const float add = row_add != nullptr ? row_add[r] : 0.f;
#pragma unroll
            for (int j = 0; j < NN; ++j) out[r * ldo + j] = acc[j] + (bias != nullptr ? bias[j] : 0.f) + add;
        }
    }
}

template <int NN, int CH>
__global__ __launch_bounds__(F_THREADS) void skinny_dgrad_kernel(long rows, int K8, const float* __restrict__ dy, long ldy,
                                                                 const float* __restrict__ w, long ldw,
                                                                 unsigned short* __restrict__ dx, long lddx, float p, float scale,
                                                                 uint64_t seed0, const uint64_t* __restrict__ epoch) {
    const int lane = threadIdx.x & (F_WAVE - 1), wave = threadIdx.x >> 6;
    const long K = (long)K8 * 8;
    float wr[NN][CH][8];
    load_weights<NN, CH>(w, ldw, K8, lane, wr);
    const bool drop = p > 0.f;
    const uint64_t seed = drop ? vb_seed_with_epoch(seed0, epoch) : 0;
    for (long r = (long)blockIdx.x * F_WAVES + wave; r < rows; r += (long)gridDim.x * F_WAVES) {
        float d[NN];
#pragma unroll
        for (int j = 0; j < NN; ++j) d[j] = dy[r * ldy + j];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + F_WAVE * i;
            if (c < K8) {
                float s[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    s[e] = d[0] * wr[0][i][e];
#pragma unroll
                    for (int j = 1; j < NN; ++j) s[e] = fmaf(d[j], wr[j][i][e], s[e]);
                }
                if (drop) drop8(s, seed, (uint64_t)(r * K + (long)c * 8), p, scale);
                *reinterpret_cast<v4i*>(dx + r * lddx + (long)c * 8) = pack8(s);
            }
        }
    }
}

// stage 1 of the weight gradient: block (= one wave) b sums the rows b * rpp .. min(rows, (b + 1) * rpp) in row order
template <int NN, int CH>
__global__ __launch_bounds__(F_WAVE) void skinny_wgrad_kernel(long rows, long rpp, int K8, const float* __restrict__ dy, long ldy,
                                                              const unsigned short* __restrict__ x, long ldx,
                                                              float* __restrict__ part, long stride, float p, float scale,
                                                              uint64_t seed0, const uint64_t* __restrict__ epoch) {
    const int lane = threadIdx.x;
    const long K = (long)K8 * 8;
    const bool drop = p > 0.f;
    const uint64_t seed = drop ? vb_seed_with_epoch(seed0, epoch) : 0;
    float acc[NN][CH][8], db[NN];
#pragma unroll
    for (int j = 0; j < NN; ++j) {
        db[j] = 0.f;
#pragma unroll
        for (int i = 0; i < CH; ++i)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[j][i][e] = 0.f;
    }
    const long r0 = (long)blockIdx.x * rpp;
    const long r1 = r0 + rpp < rows ? r0 + rpp : rows;
    for (long r = r0; r < r1; ++r) {
        const unsigned short* xr = x + r * ldx;
        float d[NN];
#pragma unroll
        for (int j = 0; j < NN; ++j) {
            d[j] = dy[r * ldy + j];
            db[j] += d[j];
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + F_WAVE * i;
            if (c < K8) {
                float f[8];
                bf16_unpack8(*reinterpret_cast<const v4i*>(xr + (long)c * 8), f);
                if (drop) drop8(f, seed, (uint64_t)(r * K + (long)c * 8), p, scale);
#pragma unroll
                for (int j = 0; j < NN; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[j][i][e] = fmaf(d[j], f[e], acc[j][i][e]);
            }
        }
    }
    float* mine = part + (long)blockIdx.x * stride;
#pragma unroll
    for (int j = 0; j < NN; ++j)
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int c = lane + F_WAVE * i;
            if (c < K8) {
                float* q = mine + (long)j * K + (long)c * 8;
                *reinterpret_cast<f32x4*>(q) = f32x4{acc[j][i][0], acc[j][i][1], acc[j][i][2], acc[j][i][3]};
                *reinterpret_cast<f32x4*>(q + 4) = f32x4{acc[j][i][4], acc[j][i][5], acc[j][i][6], acc[j][i][7]};
            }
        }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < VBF_MAX_N; ++j) mine[(long)NN * K + j] = j < NN ? db[j < NN ? j : 0] : 0.f;
    }
}

// stage 2: column c of the partial rows (c < n K: dw[c / K, c % K]; then n columns of db). Slice s of a block adds the parts
// s, s + 4, s + 8, ... in that order, the four slice sums are added as (0 + 1) + (2 + 3): a fixed order
__global__ __launch_bounds__(F_THREADS) void skinny_wgrad_reduce_kernel(long parts, int n, long K, const float* __restrict__ part,
                                                                        long stride, float* __restrict__ dw, long lddw,
                                                                        float* __restrict__ db) {
    __shared__ float red[F_RED_SLICES][F_RED_COLS];
    const int col = threadIdx.x & (F_RED_COLS - 1), slice = threadIdx.x >> 6;
    const long c = (long)blockIdx.x * F_RED_COLS + col;
    const long nk = (long)n * K;
    float a = 0.f;
    if (c < nk + n) {
#pragma unroll 4
        for (long q = slice; q < parts; q += F_RED_SLICES) a += part[q * stride + c];
    }
    red[slice][col] = a;
    __syncthreads();
    if (slice != 0 || c >= nk + n) return;
    const float total = (red[0][col] + red[1][col]) + (red[2][col] + red[3][col]);
    if (c < nk) {
        const long j = c / K;
        dw[j * lddw + (c - j * K)] += total;
    } else if (db != nullptr) {
        db[c - nk] += total;
    }
}

// fp32 rows -> bf16 rows padded with zero columns to n_pad, and per 64 rows the fp32 column sums of the UNROUNDED values: the
// identity as the producer of tile_rows16_kernel (row_kit.h), grid (ceil(rows / 64), n_pad / 64)
struct CastRows {
    static constexpr bool TRANSPOSE = false;
    const float* x; long ldx;
    __device__ float scale() const { return 1.f; }
    __device__ bool operator()(long r, int c, int n, float, float (&f)[8]) const {
        load8(x + r * ldx + c, c, n, true, f);
        return true;
    }
};

// Forward / input gradient: every wave loads the n x K fp32 weight once (from L2) and then streams its rows, so with two rows per
// wave the weight is ~25 % extra L2 traffic at n = 1 (4 KB per 2 x 2 KB of x at K = 1,024) - the price of ~6 blocks per CU at
// 12,928 rows; more rows per wave trades that against fewer waves in flight (not tried on the GPU). The weight gradient's stage 1
// runs one wave per 32 rows: ~404 waves on 256 CUs at that row count, each writing n K + 4 partial floats.
constexpr int F_ROWS_PER_BLOCK = 2 * F_WAVES;      // two rows per wave until the grid is full (F_MAX_BLOCKS)

// the checks every entry point shares: (rows, K, n), the bf16 tensor [rows, K] (stride ld16), the weight-shaped fp32 tensor
// [n, K] (stride ld32), the fp32 [rows, n] tensor (stride ldn)
int check_common(int64_t rows, int32_t K, int32_t n, const void* p16, int64_t ld16, const void* p32, int64_t ld32, const void* pn,
                 int64_t ldn, float p) {
    if (!p16 || !p32 || !pn) return VB_E_BADARG;
    if (rows < 0 || n < 1 || n > VBF_MAX_N || K < 8 || ld16 < K || ld32 < K || ldn < n) return VB_E_BADARG;
    if (!(p >= 0.f && p < 1.f)) return VB_E_BADARG;
    if (K % 8 != 0 || !vb_row16_ok(p16, ld16) || !vb_row32_ok(p32, ld32) || !vb_aligned16(pn)) return VB_E_ALIGN;
    if (K > VBF_MAX_K || rows > INT32_MAX || !vb_extent_ok(rows, ld16) || !vb_extent_ok(rows, ldn)) return VB_E_RANGE;
    return 0;
}

// KERNEL<n, chunks per lane> for the runtime (n, K): chunks = ceil(K / 512)
#define VBF_DISPATCH_CH(KERNEL, NN, GRID, BLOCK, ...)                                                                      \
    switch ((K + 511) / 512) {                                                                                             \
        case 1: hipLaunchKernelGGL((KERNEL<NN, 1>), GRID, BLOCK, 0, st, __VA_ARGS__); break;                               \
        case 2: hipLaunchKernelGGL((KERNEL<NN, 2>), GRID, BLOCK, 0, st, __VA_ARGS__); break;                               \
        case 3: hipLaunchKernelGGL((KERNEL<NN, 3>), GRID, BLOCK, 0, st, __VA_ARGS__); break;                               \
        default: hipLaunchKernelGGL((KERNEL<NN, 4>), GRID, BLOCK, 0, st, __VA_ARGS__); break;                              \
    }
#define VBF_DISPATCH(KERNEL, GRID, BLOCK, ...)                                                                             \
    switch (n) {                                                                                                           \
        case 1: VBF_DISPATCH_CH(KERNEL, 1, GRID, BLOCK, __VA_ARGS__) break;                                                \
        case 2: VBF_DISPATCH_CH(KERNEL, 2, GRID, BLOCK, __VA_ARGS__) break;                                                \
        case 3: VBF_DISPATCH_CH(KERNEL, 3, GRID, BLOCK, __VA_ARGS__) break;                                                \
        default: VBF_DISPATCH_CH(KERNEL, 4, GRID, BLOCK, __VA_ARGS__) break;                                               \
    }

}  // namespace

extern "C" int vbf_skinny_linear_fwd(void* stream, int64_t rows, int32_t K, int32_t n, const uint16_t* x, int64_t ldx,
                                     const float* w, int64_t ldw, const float* bias, const float* row_add, float* out,
                                     int64_t ldo, float p, uint64_t seed) {
    const int bad = check_common(rows, K, n, x, ldx, w, ldw, out, ldo, p);
    if (bad) return bad;
    if (!vb_aligned16(bias) || !vb_aligned16(row_add)) return VB_E_ALIGN;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(vb_grid_for(rows, F_ROWS_PER_BLOCK, F_MAX_BLOCKS));
    VBF_DISPATCH(skinny_fwd_kernel, grid, dim3(F_THREADS), (long)rows, (int)(K / 8), x, (long)ldx, w, (long)ldw,
                 bias, row_add, out, (long)ldo, p, 1.0f / (1.0f - p), seed, p > 0.f ? vb_seed_epoch() : nullptr)
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbf_skinny_linear_bwd_input(void* stream, int64_t rows, int32_t K, int32_t n, const float* dy, int64_t ldy,
                                           const float* w, int64_t ldw, uint16_t* dx, int64_t lddx, float p, uint64_t seed) {
    const int bad = check_common(rows, K, n, dx, lddx, w, ldw, dy, ldy, p);
    if (bad) return bad;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(vb_grid_for(rows, F_ROWS_PER_BLOCK, F_MAX_BLOCKS));
    VBF_DISPATCH(skinny_dgrad_kernel, grid, dim3(F_THREADS), (long)rows, (int)(K / 8), dy, (long)ldy, w, (long)ldw,
                 dx, (long)lddx, p, 1.0f / (1.0f - p), seed, p > 0.f ? vb_seed_epoch() : nullptr)
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vbf_skinny_wgrad_workspace(int64_t rows, int32_t K, int32_t n) {
    if (rows <= 0 || rows > INT32_MAX || n < 1 || n > VBF_MAX_N || K < 8 || K % 8 != 0 || K > VBF_MAX_K) return 0;
    return parts_for(rows) * ((int64_t)n * K + 4);
}

extern "C" int vbf_skinny_linear_bwd_weight(void* stream, int64_t rows, int32_t K, int32_t n, const float* dy, int64_t ldy,
                                            const uint16_t* x, int64_t ldx, float* dw, int64_t lddw, float* db, float* workspace,
                                            float p, uint64_t seed) {
    const int bad = check_common(rows, K, n, x, ldx, dw, lddw, dy, ldy, p);
    if (bad) return bad;
    if (!workspace) return VB_E_BADARG;
    if (!vb_aligned16(workspace) || !vb_aligned16(db)) return VB_E_ALIGN;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const long rpp = (rows + parts_for(rows) - 1) / parts_for(rows);     // rows per part; every launched part has rows
    const long parts = (rows + rpp - 1) / rpp;
    const long stride = (long)n * K + 4;
    VBF_DISPATCH(skinny_wgrad_kernel, dim3((unsigned)parts), dim3(F_WAVE), (long)rows, rpp, (int)(K / 8), dy, (long)ldy, x,
                 (long)ldx, workspace, stride, p, 1.0f / (1.0f - p), seed, p > 0.f ? vb_seed_epoch() : nullptr)
    VB_LAUNCH_CHECK();
    const long cols = (long)n * K + n;
    hipLaunchKernelGGL(skinny_wgrad_reduce_kernel, dim3((unsigned)((cols + F_RED_COLS - 1) / F_RED_COLS)), dim3(F_THREADS), 0, st,
                       parts, (int)n, (long)K, (const float*)workspace, stride, dw, (long)lddw, db);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbf_cast_rows_colsum(void* stream, int64_t rows, int32_t n, const float* x, int64_t ldx, uint16_t* G, int64_t ldg,
                                    float* colsum_part) {
    const long n_pad = vb_padded256(n);
    if (!x || !G || !colsum_part || rows < 0 || n < 1 || ldx < n || ldg < n_pad) return VB_E_BADARG;
    if (!vb_row32_ok(x, ldx) || !vb_row16_ok(G, ldg) || !vb_aligned16(colsum_part)) return VB_E_ALIGN;
    if (rows > F_MAX_TILED || n > F_MAX_TILED || !vb_extent_ok(rows, ldx) || !vb_extent_ok(rows, ldg)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(tile_rows16_kernel<CastRows>, dim3((unsigned)((rows + F_TILE - 1) / F_TILE), (unsigned)(n_pad / F_TILE)),
                       dim3(F_THREADS), 0, (hipStream_t)stream, (long)rows, (int)n, CastRows{x, (long)ldx}, G, (long)ldg,
                       (unsigned short*)nullptr, 0L, colsum_part, n_pad);
    VB_LAUNCH_CHECK();
    return 0;
}
