// Row kernels of an output + feed-forward block that runs on a SUBSET of its rows (vb_ffn_block.row_map; layers.hip):
//   move          out[r] = src[map[r]], 16-byte chunks of any element type  (padding rows, map[r] = -1: zeros); it serves
//                 gather and scatter here and the bf16 head rows of heads16.hip
//   drop + add    out[r] = dropout(lin[r]) + res[map[r] or r]             (the dropout / residual epilogue of the GEMMs, with
//                                                                          the mask of the FULL tensor: keep(seed, map[r] N + col);
//                                                                          without res: the dropped twin of a compact gradient)
//   invert        inv[R] = the r with map[r] == R, or -1
//   scatter       full[R] = compact[inv[R]]                               (rows no compact row stands for: zeros)
// fp32 (the mover apart), 16-byte accesses (cols % 4 == 0). The GEMM and LayerNorm kernels themselves know nothing of the map.
#include "common.h"
#include "rng.h"
#include "row_kit.h"
#include "row_map.h"

namespace {

__device__ __forceinline__ long source_row(const int32_t* __restrict__ map, long r, long src_rows) {
    const long s = map[r];
    return s >= 0 && s < src_rows ? s : -1;        // (anything outside the full tensor is a padding row)
}

// out[r] = src[map[r]] in 16-byte chunks, zeros for an entry outside the source; row strides in 16-byte units. The one mover
// of the fp32 block rows (dense) and of the bf16 head rows (strided), gather and scatter alike: a scatter is the gather through
// the inverse map.
__global__ __launch_bounds__(256) void move_rows_kernel(long rows, int chunks, const v4i* __restrict__ src, long lds,
                                                        long src_rows, const int32_t* __restrict__ map,
                                                        v4i* __restrict__ out, long ldo) {
    const long n = rows * chunks;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / chunks, c = i - r * chunks;
        const long s = source_row(map, r, src_rows);
        out[r * ldo + c] = s >= 0 ? src[s * lds + c] : v4i{0, 0, 0, 0};
    }
}

// lin and out may be the same buffer (every element is read and written by the same thread)
__global__ __launch_bounds__(256) void row_drop_add_kernel(long M, int cols4, const f32x4* lin, const f32x4* __restrict__ res,
                                                           int res_mapped, const int32_t* __restrict__ map, long src_rows,
                                                           f32x4* out, float p, float scale, uint64_t seed_in,
                                                           const uint64_t* __restrict__ epoch) {
    const uint64_t seed = p > 0.f ? vb_seed_with_epoch(seed_in, epoch) : 0;
    const long n = M * cols4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cols4, c = i - r * cols4;
        const long s = source_row(map, r, src_rows);
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (s >= 0) {
            f32x4 v = lin[i];
            if (p > 0.f) {
                const uint64_t idx = (uint64_t)((s * cols4 + c) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = vb_keep(seed, idx + e, p) ? v[e] * scale : 0.f;
            }
            o = v;
            if (res != nullptr) o += res[(res_mapped ? s : r) * cols4 + c];
        }
        out[i] = o;
    }
}

// inv[R] = the compact row that stands for full row R, or -1: one wave per full row scans the map, 64 entries per step, and
// takes the first entry that names R - every inv[R] written exactly once, no pass that clears it first, no atomics
__global__ __launch_bounds__(256) void invert_map_kernel(long src_rows, int M, const int32_t* __restrict__ map,
                                                         int32_t* __restrict__ inv) {
    const int lane = threadIdx.x & 63;
    const long R = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (R >= src_rows) return;
    int found = -1;
    for (int base = 0; base < M && found < 0; base += 64) {
        const int r = base + lane;
        const unsigned long long hits = __ballot(r < M && (long)map[r] == R);
        if (hits != 0) found = base + __ffsll(hits) - 1;
    }
    if (lane == 0) inv[R] = found;
}

constexpr long ROW_MAX_BLOCKS = 2048;

}  // namespace

namespace vbrows {

int move_rows(hipStream_t st, long rows, int chunks, const void* src, long lds, long src_rows, const int32_t* map, void* out,
              long ldo, long max_blocks) {
    hipLaunchKernelGGL(move_rows_kernel, dim3(vb_grid_for(rows * chunks, 256, max_blocks)), dim3(256), 0, st, rows, chunks,
                       static_cast<const v4i*>(src), lds, src_rows, map, static_cast<v4i*>(out), ldo);
    VB_LAUNCH_CHECK();
    return 0;
}

int gather(hipStream_t st, long M, int cols, const float* src, const int32_t* map, long src_rows, float* out) {
    return move_rows(st, M, cols / 4, src, cols / 4, src_rows, map, out, cols / 4, ROW_MAX_BLOCKS);
}

int drop_add(hipStream_t st, long M, int cols, const float* lin, const float* res, bool res_mapped, const int32_t* map,
             long src_rows, float* out, float p, uint64_t seed) {
    hipLaunchKernelGGL(row_drop_add_kernel, dim3(vb_grid_for(M * (cols / 4), 256, ROW_MAX_BLOCKS)), dim3(256), 0, st, M, cols / 4,
                       reinterpret_cast<const f32x4*>(lin), reinterpret_cast<const f32x4*>(res), res_mapped ? 1 : 0, map, src_rows,
                       reinterpret_cast<f32x4*>(out), p, 1.0f / (1.0f - p), seed, p > 0.f ? vb_seed_epoch() : nullptr);
    VB_LAUNCH_CHECK();
    return 0;
}

int invert(hipStream_t st, long src_rows, long M, const int32_t* map, int32_t* inv) {
    hipLaunchKernelGGL(invert_map_kernel, dim3((unsigned)((src_rows + 3) / 4)), dim3(256), 0, st, src_rows, (int)M, map, inv);
    VB_LAUNCH_CHECK();
    return 0;
}

int scatter(hipStream_t st, long src_rows, int cols, const float* compact, long M, const int32_t* inv, float* full) {
    return move_rows(st, src_rows, cols / 4, compact, cols / 4, M, inv, full, cols / 4, ROW_MAX_BLOCKS);
}

}  // namespace vbrows
