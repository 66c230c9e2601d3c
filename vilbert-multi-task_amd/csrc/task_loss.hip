// Loss and answer score of the fine-tuning heads (vilbert/task_utils.py:25-28, 325-374, 618-623 of the reference):
//  * nn.BCEWithLogitsLoss(reduction="mean") on [rows, n] fp32 logits and soft targets, forward and backward
//    (VQA / GenomeQA / GQA answers n = 3129 | 1533, Visual7w / refcoco region logits, NLVR2 n = 2, SNLI-VE n = 3);
//  * compute_score_with_logits: per row the arg-max of the logits, the label there, and (optionally) the dense
//    one-hot-times-labels matrix the reference returns.
// Every operand is read once per direction. Two mappings, chosen by the row width alone (BCE_ROW_MIN_N):
//    n <  256  flat: the rows * n elements are spread over the grid 1024 per block, whatever the row count - the binary /
//              tri heads have 2 - 3 columns and many rows, a block per row would idle 253 lanes of 256;
//              (the arg-max gives each row one 64-lane wave, four rows to a block)
//    n >= 256  one 256-thread block per row (grid-strided over the rows beyond the grid cap), as loss.hip does.
// The forward is deterministic: no floating-point atomics - each block stores ONE partial sum to the caller's workspace
// and a single block adds the partials in index order; a launch that needs one block only writes the loss itself.
#include "common.h"
#include "row_kit.h"

#include "../../include/vilbert_hip_tasks.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int BCE_ROW_MIN_N = 256;          // rows at least this wide get a block each
constexpr int BCE_FLAT_PER_BLOCK = 1024;    // elements a block of the flat mapping takes per grid stride (4 per thread)
constexpr long BCE_MAX_PARTIALS = 1024;     // grid cap of the forward = workspace floats
constexpr long BCE_BWD_MAX_BLOCKS = 65536;

// max(x, 0) - x t + log(1 + exp(-|x|)): exp never sees a positive argument, so nothing overflows at any x
__device__ __forceinline__ float bce_term(float x, float t) {
    return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
}

// sigmoid(x) from exp(-|x|) in (0, 1]: 1 / (1 + e) for x >= 0, e / (1 + e) below
__device__ __forceinline__ float stable_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    const float r = 1.f / (1.f + e);
    return x >= 0.f ? r : e * r;
}

__device__ __forceinline__ void bce_store_partial(float s, float inv_count, float* __restrict__ partials,
                                                  float* __restrict__ loss) {
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) loss[0] = s * inv_count;
        else partials[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(TL_THREADS) void bce_fwd_flat_kernel(long total, int n, const float* __restrict__ logits,
                                                                  long ld, const float* __restrict__ target, long ldt,
                                                                  float inv_count, float* __restrict__ partials,
                                                                  float* __restrict__ loss) {
    __shared__ float scratch[TL_THREADS / 64];
    const bool dense = ld == n && ldt == n;          // grid-uniform: no division on contiguous operands
    float s = 0.f;
    for (long i = (long)blockIdx.x * TL_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * TL_THREADS) {
        long ox = i, ot = i;
        if (!dense) {
            const long r = i / n;
            const long j = i - r * n;
            ox = r * ld + j;
            ot = r * ldt + j;
        }
        s += bce_term(logits[ox], target[ot]);
    }
    s = block_reduce<false, TL_THREADS>(s, scratch);
    bce_store_partial(s, inv_count, partials, loss);
}

__global__ __launch_bounds__(TL_THREADS) void bce_fwd_rows_kernel(long rows, int n, const float* __restrict__ logits,
                                                                  long ld, const float* __restrict__ target, long ldt,
                                                                  float inv_count, float* __restrict__ partials,
                                                                  float* __restrict__ loss) {
    __shared__ float scratch[TL_THREADS / 64];
    float s = 0.f;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* x = logits + r * ld;
        const float* t = target + r * ldt;
        for (int j = threadIdx.x; j < n; j += TL_THREADS) s += bce_term(x[j], t[j]);
    }
    s = block_reduce<false, TL_THREADS>(s, scratch);
    bce_store_partial(s, inv_count, partials, loss);
}

// loss = inv_count * (partials[0] + partials[1] + ...): thread k adds partials k, k + 256, ... in that order, then the fixed
// tree of block_reduce - the same association on every run
__global__ __launch_bounds__(TL_THREADS) void bce_finish_kernel(int n_partials, const float* __restrict__ partials,
                                                                float inv_count, float* __restrict__ loss) {
    __shared__ float scratch[TL_THREADS / 64];
    float s = 0.f;
    for (int i = threadIdx.x; i < n_partials; i += TL_THREADS) s += partials[i];
    s = block_reduce<false, TL_THREADS>(s, scratch);
    if (threadIdx.x == 0) loss[0] = s * inv_count;
}

__global__ __launch_bounds__(TL_THREADS) void bce_bwd_flat_kernel(long total, int n, const float* __restrict__ logits,
                                                                  long ld, const float* __restrict__ target, long ldt,
                                                                  const float* __restrict__ gout, float inv_count,
                                                                  float* __restrict__ dlogits, long ldd) {
    const bool dense = ld == n && ldt == n && ldd == n;
    const float g = gout[0] * inv_count;
    for (long i = (long)blockIdx.x * TL_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * TL_THREADS) {
        long ox = i, ot = i, od = i;
        if (!dense) {
            const long r = i / n;
            const long j = i - r * n;
            ox = r * ld + j;
            ot = r * ldt + j;
            od = r * ldd + j;
        }
        dlogits[od] = (stable_sigmoid(logits[ox]) - target[ot]) * g;
    }
}

__global__ __launch_bounds__(TL_THREADS) void bce_bwd_rows_kernel(long rows, int n, const float* __restrict__ logits,
                                                                  long ld, const float* __restrict__ target, long ldt,
                                                                  const float* __restrict__ gout, float inv_count,
                                                                  float* __restrict__ dlogits, long ldd) {
    const float g = gout[0] * inv_count;
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* x = logits + r * ld;
        const float* t = target + r * ldt;
        float* d = dlogits + r * ldd;
        for (int j = threadIdx.x; j < n; j += TL_THREADS) d[j] = (stable_sigmoid(x[j]) - t[j]) * g;
    }
}

// torch.max's order: a NaN beats every number, among equals (two NaNs included) the lower index wins
__device__ __forceinline__ bool arg_better(float a, int ia, float b, int ib) {
    const bool an = a != a, bn = b != b;
    if (an != bn) return an;
    if (!an && a != b) return a > b;
    return ia < ib;
}

// GROUP threads per row (64 = one wave, no LDS; 256 = the whole block), TL_THREADS / GROUP rows per block
template <int GROUP>
__global__ __launch_bounds__(TL_THREADS) void argmax_pick_kernel(long rows, int n, const float* __restrict__ logits, long ld,
                                                                 const float* __restrict__ labels, long ldl,
                                                                 int64_t* __restrict__ idx_out, float* __restrict__ picked,
                                                                 float* __restrict__ dense, long ldo) {
    constexpr int ROWS_PER_BLOCK = TL_THREADS / GROUP;
    const int lane = threadIdx.x % GROUP;
    const long r = (long)blockIdx.x * ROWS_PER_BLOCK + threadIdx.x / GROUP;
    if (GROUP == 64 && r >= rows) return;          // whole waves leave; the 256-wide variant has exactly one row per block
    const float* x = logits + r * ld;
    float best = -INFINITY;
    int bi = n;                                     // "nothing seen": loses every tie
    for (int j = lane; j < n; j += GROUP) {
        const float v = x[j];
        if (arg_better(v, j, best, bi)) { best = v; bi = j; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(best, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (arg_better(ov, oi, best, bi)) { best = ov; bi = oi; }
    }
    if (GROUP > 64) {
        __shared__ float s_v[TL_THREADS / 64];
        __shared__ int s_i[TL_THREADS / 64];
        if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = best; s_i[threadIdx.x >> 6] = bi; }
        __syncthreads();
        best = s_v[0];
        bi = s_i[0];
#pragma unroll
        for (int w = 1; w < TL_THREADS / 64; ++w)
            if (arg_better(s_v[w], s_i[w], best, bi)) { best = s_v[w]; bi = s_i[w]; }
    }
    // a row of -inf only: every element ties with the start value and the lowest index 0 was taken (bi < n always)
    const float lab = labels[r * ldl + bi];
    if (lane == 0) {
        idx_out[r] = bi;
        picked[r] = lab;
    }
    if (dense != nullptr) {
        float* o = dense + r * ldo;
        for (int j = lane; j < n; j += GROUP) o[j] = j == bi ? lab : 0.f;
    }
}

inline long bce_fwd_blocks(int64_t rows, int32_t n) {
    if (n >= BCE_ROW_MIN_N) return rows < BCE_MAX_PARTIALS ? rows : BCE_MAX_PARTIALS;
    const int64_t b = (rows * n + BCE_FLAT_PER_BLOCK - 1) / BCE_FLAT_PER_BLOCK;
    return b < BCE_MAX_PARTIALS ? b : BCE_MAX_PARTIALS;
}

}  // namespace

extern "C" int64_t vbt_bce_workspace(int64_t rows, int32_t n) {
    if (rows <= 0 || n <= 0 || !vb_extent_ok(rows, n)) return 0;
    return bce_fwd_blocks(rows, n);
}

extern "C" int vbt_bce_fwd(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const float* target,
                           int64_t ldt, float* workspace, float* loss) {
    if (rows < 0 || n <= 0 || ld < n || ldt < n) return VB_E_BADARG;
    if (!logits || !target || !workspace || !loss) return VB_E_BADARG;
    if (!vb_extent_ok(rows, ld) || !vb_extent_ok(rows, ldt)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const long blocks = bce_fwd_blocks(rows, n);
    const float inv_count = (float)(1.0 / ((double)rows * (double)n));
    if (n >= BCE_ROW_MIN_N)
        hipLaunchKernelGGL(bce_fwd_rows_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, st, (long)rows, n, logits,
                           (long)ld, target, (long)ldt, inv_count, workspace, loss);
    else
        hipLaunchKernelGGL(bce_fwd_flat_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, st, (long)(rows * n), n, logits,
                           (long)ld, target, (long)ldt, inv_count, workspace, loss);
    VB_LAUNCH_CHECK();
    if (blocks > 1) {
        hipLaunchKernelGGL(bce_finish_kernel, dim3(1), dim3(TL_THREADS), 0, st, (int)blocks, workspace, inv_count, loss);
        VB_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int vbt_bce_bwd(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const float* target,
                           int64_t ldt, const float* grad_loss, float* dlogits, int64_t ldd) {
    if (rows < 0 || n <= 0 || ld < n || ldt < n || ldd < n) return VB_E_BADARG;
    if (!logits || !target || !grad_loss || !dlogits) return VB_E_BADARG;
    if (!vb_extent_ok(rows, ld) || !vb_extent_ok(rows, ldt) || !vb_extent_ok(rows, ldd)) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const float inv_count = (float)(1.0 / ((double)rows * (double)n));
    if (n >= BCE_ROW_MIN_N) {
        const long blocks = rows < BCE_BWD_MAX_BLOCKS ? rows : BCE_BWD_MAX_BLOCKS;
        hipLaunchKernelGGL(bce_bwd_rows_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, st, (long)rows, n, logits,
                           (long)ld, target, (long)ldt, grad_loss, inv_count, dlogits, (long)ldd);
    } else {
        const int64_t total = rows * n;
        int64_t blocks = (total + BCE_FLAT_PER_BLOCK - 1) / BCE_FLAT_PER_BLOCK;
        if (blocks > BCE_BWD_MAX_BLOCKS) blocks = BCE_BWD_MAX_BLOCKS;
        hipLaunchKernelGGL(bce_bwd_flat_kernel, dim3((unsigned)blocks), dim3(TL_THREADS), 0, st, (long)total, n, logits,
                           (long)ld, target, (long)ldt, grad_loss, inv_count, dlogits, (long)ldd);
    }
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbt_argmax_pick(void* stream, int64_t rows, int32_t n, const float* logits, int64_t ld, const float* labels,
                               int64_t ldl, int64_t* idx, float* picked, float* dense, int64_t ldo) {
    if (rows < 0 || n <= 0 || ld < n || ldl < n || (dense != nullptr && ldo < n)) return VB_E_BADARG;
    if (!logits || !labels || !idx || !picked) return VB_E_BADARG;
    if (!vb_extent_ok(rows, ld) || !vb_extent_ok(rows, ldl) || (dense != nullptr && !vb_extent_ok(rows, ldo))) return VB_E_RANGE;
    if (rows > (int64_t)INT32_MAX) return VB_E_RANGE;          // one block per row in the wide mapping: the grid's x extent
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n >= BCE_ROW_MIN_N)
        hipLaunchKernelGGL(argmax_pick_kernel<TL_THREADS>, dim3((unsigned)rows), dim3(TL_THREADS), 0, st, (long)rows, n, logits,
                           (long)ld, labels, (long)ldl, idx, picked, dense, (long)ldo);
    else
        hipLaunchKernelGGL(argmax_pick_kernel<64>, dim3((unsigned)((rows + 3) / 4)), dim3(TL_THREADS), 0, st, (long)rows, n,
                           logits, (long)ld, labels, (long)ldl, idx, picked, dense, (long)ldo);
    VB_LAUNCH_CHECK();
    return 0;
}
