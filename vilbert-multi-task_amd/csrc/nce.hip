// NCE masked-region loss of pre-training, visual_target == 2 (reference vilbert.py:1523-1575): every labelled region's
// predicted feature is scored against its own target feature and n_neg sampled rows of the flat target table, cross entropy
// with class 0 over the 1 + n_neg scores. The reference gathers a [rows, 1 + n_neg, dim] tensor (1.45 GB at 1,380 rows x 129
// candidates x 2048), concatenates it (a second copy) and feeds it to a bmm; here the candidate rows are read where they lie.
//
//  * nce_negatives_kernel: the index table, one thread per entry (nce_index.h - the function the host restates).
//  * nce_fwd_kernel: one 256-thread block per labelled row (grid-strided beyond the grid cap).
//      pass 1  a WAVE per candidate: each lane keeps its 32 elements of predict[r] in registers (dim <= 2048; the rest is
//              re-read) and takes 16 bytes per load, the wave 1 KB of the candidate row per instruction, 8 independent loads
//              in flight per candidate; the wave's sum is the score, kept in LDS.
//      softmax max / sum over the scores in LDS (block reductions of a fixed shape), row loss, weights p_c - [c == 0].
//      pass 2  (only when the gradient is wanted) a THREAD per 4 columns, all candidates in index order: dsave[r, :] = sum_c
//              w_c table[cand_c, :] without any cross-thread reduction - the same association for every dim and grid. The
//              1 + n_neg rows (1 - 2 MB at the pre-training shape) were read by this block a moment ago: L2 hits.
//      The row losses of a block's rows are added in row order into ONE partial per block.
//  * nce_finish_kernel: the partials in index order, divided by the device-side count.
//  * nce_bwd_kernel: dpredict = grad / count * dsave, exact zeros on invalid rows.
// Indices come from device memory: a candidate outside the table is never followed (its score becomes NaN).
#include "common.h"
#include "nce_index.h"
#include "rng.h"
#include "row_kit.h"

#include "../../include/vilbert_hip_pretrain.h"

namespace {

constexpr int NCE_THREADS = 256;
constexpr int NCE_WAVES = NCE_THREADS / 64;
constexpr long NCE_MAX_BLOCKS = 4096;       // grid cap of the forward = workspace floats
constexpr int NCE_MAX_NEG = 4095;           // 1 + n_neg candidates x 12 bytes of LDS (offset + weight) <= 48 KB
constexpr int NCE_REG_VEC = 8;              // float4 of predict a lane keeps: 8 x 4 x 64 lanes = 2048 columns
constexpr long NCE_BWD_MAX_BLOCKS = 65536;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}

__global__ __launch_bounds__(NCE_THREADS) void nce_negatives_kernel(long total, int n_neg, const int64_t* __restrict__ region,
                                                                    int batch, int regions, int n_across, int n_inside,
                                                                    uint64_t seed_in, const uint64_t* __restrict__ epoch,
                                                                    int64_t* __restrict__ out) {
    const uint64_t seed = vb_seed_with_epoch(seed_in, epoch);
    const long n_table = (long)batch * regions;
    for (long i = (long)blockIdx.x * NCE_THREADS + threadIdx.x; i < total; i += (long)gridDim.x * NCE_THREADS) {
        const long row = i / n_neg;
        const int j = (int)(i - row * n_neg);
        const int64_t g = region[row];
        out[i] = (g >= 0 && g < n_table) ? vbnce::negative_row(seed, g, j, batch, regions, n_across, n_inside) : -1;
    }
}

// dynamic LDS: long s_off[C] (element offset of candidate c's row in the table; 0 for an index outside it), then float s_w[C]
// (pass 1: the score; pass 2: the weight; NaN for an index outside the table)
template <bool VEC>
__global__ __launch_bounds__(NCE_THREADS) void nce_fwd_kernel(long rows, int dim, int n_neg, const float* __restrict__ predict,
                                                              long ldp, const float* __restrict__ table, long table_rows,
                                                              long ldt, const int64_t* __restrict__ pos_idx,
                                                              const int64_t* __restrict__ neg_idx,
                                                              const uint8_t* __restrict__ valid, const float* __restrict__ count,
                                                              float* __restrict__ partials, float* __restrict__ loss,
                                                              float* __restrict__ dsave, long lds) {
    extern __shared__ long s_dyn[];
    __shared__ float scratch[NCE_WAVES];
    const int C = 1 + n_neg;
    long* s_off = s_dyn;
    float* s_w = reinterpret_cast<float*>(s_dyn + C);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dim4 = VEC ? (dim & ~3) : 0;          // columns served by 16-byte accesses; the rest one by one
    float block_loss = 0.f;

    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        if (valid != nullptr && valid[r] == 0) {    // block-uniform
            if (dsave != nullptr)
                for (int j = tid; j < dim; j += NCE_THREADS) dsave[r * lds + j] = 0.f;
            continue;
        }
        const float* p = predict + r * ldp;
        __syncthreads();                            // the previous row's pass 2 is done with s_off / s_w
        for (int c = tid; c < C; c += NCE_THREADS) {
            const int64_t idx = c == 0 ? pos_idx[r] : neg_idx[r * n_neg + (c - 1)];
            const bool ok = idx >= 0 && idx < table_rows;
            s_off[c] = ok ? idx * ldt : 0;
            s_w[c] = ok ? 0.f : NAN;
        }
        f32x4 pr[NCE_REG_VEC];
#pragma unroll
        for (int k = 0; k < NCE_REG_VEC; ++k) {
            const int j = k * 256 + lane * 4;
            pr[k] = j < dim4 ? ld4(p + j) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();

        // ---- pass 1: scores
        for (int c = wave; c < C; c += NCE_WAVES) {
            const float* t = table + s_off[c];
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < NCE_REG_VEC; ++k) {
                const int j = k * 256 + lane * 4;
                if (j < dim4) acc = dot4(ld4(t + j), pr[k], acc);
            }
            for (int j = NCE_REG_VEC * 256 + lane * 4; j < dim4; j += 256) acc = dot4(ld4(t + j), ld4(p + j), acc);
            for (int j = dim4 + lane; j < dim; j += 64) acc = fmaf(t[j], p[j], acc);
            acc = wave_sum(acc);
            if (lane == 0) s_w[c] += acc;           // 0 + score, or NaN + score = NaN
        }
        __syncthreads();

        // ---- log-sum-exp over the C scores
        float m = -INFINITY;
        for (int c = tid; c < C; c += NCE_THREADS) m = fmaxf(m, s_w[c]);   // (fmaxf drops a NaN; the sum below keeps it)
        m = block_reduce<true, NCE_THREADS>(m, scratch);
        float e = 0.f;
        for (int c = tid; c < C; c += NCE_THREADS) e += expf(s_w[c] - m);
        e = block_reduce<false, NCE_THREADS>(e, scratch);
        const float lse = m + logf(e);
        block_loss += lse - s_w[0];                 // every thread holds the same value
        if (dsave == nullptr) continue;
        __syncthreads();                            // everyone has read s_w[0]
        // softmax as exp(s - max) / sum, not exp(s - lse): the rounding of lse would be magnified by |lse|
        for (int c = tid; c < C; c += NCE_THREADS) s_w[c] = expf(s_w[c] - m) / e - (c == 0 ? 1.f : 0.f);
        __syncthreads();

        // ---- pass 2: dsave[r, j] = sum_c w_c table[cand_c, j], c in index order
        float* d = dsave + r * lds;
        for (int j0 = 0; j0 < dim4; j0 += 2 * NCE_THREADS * 4) {
            const int ja = j0 + tid * 4, jb = ja + NCE_THREADS * 4;
            const bool ha = ja < dim4, hb = jb < dim4;
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int c = 0; c < C; ++c) {
                const float* t = table + s_off[c];
                const float w = s_w[c];
                if (ha) a += w * ld4(t + ja);
                if (hb) b += w * ld4(t + jb);
            }
            if (ha) *reinterpret_cast<f32x4*>(d + ja) = a;
            if (hb) *reinterpret_cast<f32x4*>(d + jb) = b;
        }
        for (int j = dim4 + tid; j < dim; j += NCE_THREADS) {
            float a = 0.f;
            for (int c = 0; c < C; ++c) a = fmaf(s_w[c], table[s_off[c] + j], a);
            d[j] = a;
        }
    }
    if (tid == 0) {
        if (gridDim.x == 1) loss[0] = block_loss / count[0];
        else partials[blockIdx.x] = block_loss;
    }
}

// loss = (partials[0] + partials[1] + ...) / count: thread k adds partials k, k + 256, ... in that order, then the fixed tree of
// block_reduce - the same association on every run
__global__ __launch_bounds__(NCE_THREADS) void nce_finish_kernel(int n_partials, const float* __restrict__ partials,
                                                                 const float* __restrict__ count, float* __restrict__ loss) {
    __shared__ float scratch[NCE_WAVES];
    float s = 0.f;
    for (int i = threadIdx.x; i < n_partials; i += NCE_THREADS) s += partials[i];
    s = block_reduce<false, NCE_THREADS>(s, scratch);
    if (threadIdx.x == 0) loss[0] = s / count[0];
}

__global__ __launch_bounds__(NCE_THREADS) void nce_bwd_kernel(long rows, int dim, const float* __restrict__ dsave, long lds,
                                                              const uint8_t* __restrict__ valid, const float* __restrict__ gout,
                                                              const float* __restrict__ count, float* __restrict__ dpredict,
                                                              long ldd) {
    const float g = gout[0] / count[0];
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const bool on = valid == nullptr || valid[r] != 0;
        const float* s = dsave + r * lds;
        float* d = dpredict + r * ldd;
        if (on)
            for (int j = threadIdx.x; j < dim; j += NCE_THREADS) d[j] = g * s[j];
        else
            for (int j = threadIdx.x; j < dim; j += NCE_THREADS) d[j] = 0.f;
    }
}

}  // namespace

extern "C" int vbp_nce_negatives(void* stream, int64_t rows, const int64_t* region_idx, int32_t batch, int32_t regions,
                                 int32_t n_across, int32_t n_inside, uint64_t seed, int64_t* neg_idx) {
    if (rows < 0 || batch < 1 || regions < 1 || n_across < 0 || n_inside < 0) return VB_E_BADARG;
    const int64_t n_neg = (int64_t)n_across + (int64_t)n_inside;
    if (n_neg < 1 || (n_across > 0 && batch < 2) || (n_inside > 0 && regions < 2)) return VB_E_BADARG;
    if (!region_idx || !neg_idx) return VB_E_BADARG;
    if (n_neg > INT32_MAX || !vb_extent_ok(rows, 2 * n_neg) || !vb_extent_ok((int64_t)batch * regions, 2 * n_neg)) return VB_E_RANGE;
    if (rows == 0) return 0;
    const int64_t total = rows * n_neg;
    int64_t blocks = (total + NCE_THREADS - 1) / NCE_THREADS;
    if (blocks > NCE_BWD_MAX_BLOCKS) blocks = NCE_BWD_MAX_BLOCKS;
    hipLaunchKernelGGL(nce_negatives_kernel, dim3((unsigned)blocks), dim3(NCE_THREADS), 0, (hipStream_t)stream, (long)total,
                       (int)n_neg, region_idx, batch, regions, n_across, n_inside, seed, vb_seed_epoch(), neg_idx);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vbp_nce_workspace(int64_t rows) {
    if (rows <= 0) return 0;
    return rows < NCE_MAX_BLOCKS ? rows : NCE_MAX_BLOCKS;
}

extern "C" int vbp_nce_fwd(void* stream, int64_t rows, int32_t dim, int32_t n_neg, const float* predict, int64_t ldp,
                           const float* table, int64_t table_rows, int64_t ldt, const int64_t* pos_idx, const int64_t* neg_idx,
                           const uint8_t* valid, const float* count, float* workspace, float* loss, float* dsave, int64_t lds) {
    if (rows < 0 || dim < 1 || n_neg < 1 || table_rows < 1 || ldp < dim || ldt < dim || (dsave != nullptr && lds < dim))
        return VB_E_BADARG;
    if (!predict || !table || !pos_idx || !neg_idx || !count || !workspace || !loss) return VB_E_BADARG;
    if (n_neg > NCE_MAX_NEG || !vb_extent_ok(rows, ldp) || !vb_extent_ok(rows, n_neg) || !vb_extent_ok(table_rows, ldt) ||
        (dsave != nullptr && !vb_extent_ok(rows, lds)))
        return VB_E_RANGE;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const long blocks = rows < NCE_MAX_BLOCKS ? rows : NCE_MAX_BLOCKS;
    const size_t lds_bytes = (size_t)(1 + n_neg) * (sizeof(long) + sizeof(float));
    const bool vec = vb_row32_ok(predict, ldp) && vb_row32_ok(table, ldt) && (dsave == nullptr || vb_row32_ok(dsave, lds));
    if (vec)
        hipLaunchKernelGGL(nce_fwd_kernel<true>, dim3((unsigned)blocks), dim3(NCE_THREADS), lds_bytes, st, (long)rows, dim, n_neg,
                           predict, (long)ldp, table, (long)table_rows, (long)ldt, pos_idx, neg_idx, valid, count, workspace, loss,
                           dsave, (long)lds);
    else
        hipLaunchKernelGGL(nce_fwd_kernel<false>, dim3((unsigned)blocks), dim3(NCE_THREADS), lds_bytes, st, (long)rows, dim, n_neg,
                           predict, (long)ldp, table, (long)table_rows, (long)ldt, pos_idx, neg_idx, valid, count, workspace, loss,
                           dsave, (long)lds);
    VB_LAUNCH_CHECK();
    if (blocks > 1) {
        hipLaunchKernelGGL(nce_finish_kernel, dim3(1), dim3(NCE_THREADS), 0, st, (int)blocks, workspace, count, loss);
        VB_LAUNCH_CHECK();
    }
    return 0;
}

extern "C" int vbp_nce_bwd(void* stream, int64_t rows, int32_t dim, const float* dsave, int64_t lds, const uint8_t* valid,
                           const float* grad_loss, const float* count, float* dpredict, int64_t ldd) {
    if (rows < 0 || dim < 1 || lds < dim || ldd < dim) return VB_E_BADARG;
    if (!dsave || !grad_loss || !count || !dpredict) return VB_E_BADARG;
    if (!vb_extent_ok(rows, lds) || !vb_extent_ok(rows, ldd)) return VB_E_RANGE;
    if (rows == 0) return 0;
    const long blocks = rows < NCE_BWD_MAX_BLOCKS ? rows : NCE_BWD_MAX_BLOCKS;
    hipLaunchKernelGGL(nce_bwd_kernel, dim3((unsigned)blocks), dim3(NCE_THREADS), 0, (hipStream_t)stream, (long)rows, dim, dsave,
                       (long)lds, valid, grad_loss, count, dpredict, (long)ldd);
    VB_LAUNCH_CHECK();
    return 0;
}
