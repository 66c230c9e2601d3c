// The feature-row kernels of the batch-finishing calls, ONE body per call for every input / output element type: the
// Conceptual-Captions block (batch.hip: vbw_concap_finish_batch; the fp32 call vb_concap_finish_batch keeps a kernel of its own
// there, see below) and the padded block of a fine-tuning batch built from packed regions (task_batch.hip:
// vbd_task_finish_batch, vbw_task_finish_batch). A thread owns one 16-byte column group of its input - 4 fp32 or 8 binary16
// columns - widens a row as it is read and rounds it as it is stored; the loads of ROWS rows are issued before the first of them
// is used and only the adds are serial. The arithmetic is stated here: the column sums run in row order with one __fadd_rn per
// row, the Conceptual-Captions mean divides in fp64 by the count, the fine-tuning mean in fp32 with __fdiv_rn, and the numpy
// restatements pin every bit (oracle/batch_oracle.py, tests/task_batch_restatement.py) - so nothing here is contracted into a
// fused multiply-add.
#pragma once
#include "common.h"
#include "task_rows.h"

#pragma clang fp contract(off)

namespace vbfeat {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct bf16 {   // element of a bf16 feature output (rounded by vb_bf16_pack); an fp32 output has `float` elements
    uint16_t bits;
};

// The column group of a thread per input element type: Raw = one 16-byte load, Wide = its N exact fp32 values, store writes
// them to the N output elements at p (16-byte aligned), rounded to the element type of p. THREADS / ROWS:
// block size and the independent loads a thread has in flight, per kernel.
// The kernels address an output row as base + (element index): with a pointer advanced per row instead, hipcc allocates the bf16
// kernels differently (68 / 94 instead of 98 / 128 VGPRs) and both measure 0.5 us slower (profiles/feat_rows_ab.txt).
template <typename In>
struct Cols;

template <>
struct Cols<float> {
    typedef f32x4 Raw;
    typedef f32x4 Wide;
    static constexpr int N = 4;
    static constexpr int TASK_THREADS = 64, TASK_ROWS = 8;        // one wave owns 256 columns: 8 blocks per sample at F = 2048
    static __device__ __forceinline__ Wide widen(Raw v) { return v; }
    static __device__ __forceinline__ void store(float* p, Wide v) { *reinterpret_cast<f32x4*>(p) = v; }   // no bf16 output
};

template <>
struct Cols<_Float16> {
    typedef f16x8 Raw;
    typedef f32x8 Wide;
    static constexpr int N = 8;
    static constexpr int TASK_THREADS = 64, TASK_ROWS = 8;        // one wave owns 512 columns: 4 blocks per sample at F = 2048
    static constexpr int CONCAP_THREADS = 64, CONCAP_ROWS = 8;
    // binary16 -> fp32 is exact (v_cvt_f32_f16; the kernels run with denormals on: subnormals keep their value)
    static __device__ __forceinline__ Wide widen(Raw h) { return __builtin_convertvector(h, f32x8); }
    static __device__ __forceinline__ void store(float* p, Wide v) {
        const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4*>(p) = lo;
        *reinterpret_cast<f32x4*>(p + 4) = hi;
    }
    static __device__ __forceinline__ void store(bf16* p, Wide v) {
        u32x4 w;
        w[0] = vb_bf16_pack(v[0], v[1]);
        w[1] = vb_bf16_pack(v[2], v[3]);
        w[2] = vb_bf16_pack(v[4], v[5]);
        w[3] = vb_bf16_pack(v[6], v[7]);
        *reinterpret_cast<u32x4*>(p) = w;
    }
};

// Conceptual-Captions: out[b, r + 1, c] = x[b, r, c], out[b, 0, c] = sum_r x / count, where x[b, r] is the widened input row, or
// zeros where zero_row (optional) flags it - such a row is not loaded and adds its +0, as a cleared fp32 row does. The sum runs
// over r = 0 .. R - 1 in fp32 in that order (numpy's np.sum(x, axis=1) of a C-contiguous [B, R, F] array adds the R rows in
// order); count = max(#(masked_label[b, :] == 0), 1) and the division is done in fp64 and rounded to fp32, exactly like
// `np.sum(..) / sum_count` (float32 / int64 -> float64) followed by the float32 cast (concept_cap_dataset.py:251-256).
// Grid: x = column groups, y = samples (batch-strided). Instantiated for binary16 input only: the fp32 instantiation (256
// threads, 4 rows in flight) measured 0.3 - 0.9 us (1 - 2 %) behind batch.hip's plain row loop at 256 x 36 x 2048
// (profiles/feat_rows_ab.txt), so the fp32 call keeps that kernel, which states this arithmetic a second time.
template <typename In, typename Out>
__global__ __launch_bounds__(Cols<In>::CONCAP_THREADS) void concap_feat_kernel(int B, int R, int F, const In* __restrict__ in,
                                                                               const int64_t* __restrict__ masked_label,
                                                                               const uint8_t* __restrict__ zero_row,
                                                                               void* __restrict__ out) {
    typedef Cols<In> G;
    constexpr int ROWS = G::CONCAP_ROWS;
    const long c = ((long)blockIdx.x * G::CONCAP_THREADS + threadIdx.x) * G::N;
    if (c >= F) return;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        int cnt = 0;
        for (int r = 0; r < R; ++r) cnt += masked_label[b * R + r] == 0 ? 1 : 0;
        if (cnt == 0) cnt = 1;
        const In* src = in + b * R * F + c;
        const uint8_t* flags = zero_row != nullptr ? zero_row + b * R : nullptr;
        Out* const o = static_cast<Out*>(out);
        const long dst = b * (R + 1) * F + c;
        typename G::Wide s = {};
        for (int r0 = 0; r0 < R; r0 += ROWS) {
            typename G::Raw h[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                h[u] = typename G::Raw{};
                const int r = r0 + u;
                if (r < R && (flags == nullptr || flags[r] == 0))
                    h[u] = *reinterpret_cast<const typename G::Raw*>(src + (long)r * F);
            }
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                const int r = r0 + u;
                if (r < R) {
                    const typename G::Wide v = G::widen(h[u]);
                    G::store(o + (dst + (long)(r + 1) * F), v);
#pragma unroll
                    for (int e = 0; e < G::N; ++e) s[e] = __fadd_rn(s[e], v[e]);
                }
            }
        }
        typename G::Wide g;
#pragma unroll
        for (int e = 0; e < G::N; ++e) g[e] = (float)((double)s[e] / (double)cnt);
        G::store(o + dst, g);
    }
}

// Where the rows of output sample b come from, per argument struct. image(a, b): the index of the sample's per-image words
// (image_wh, mean_rows), or < 0 for a sample that owns nothing - such a sample reads none of them; span(a, img): its clamped
// rows. The per-batch words (ref_box, the outputs) are always indexed by b.
// This one: a packed fine-tuning batch (vbd_task_batch or vbw_task_batch), whose sample b is image b. region_store.hip
// specialises it for a device-resident store, whose samples name their image by an id word.
template <typename Args>
struct Source {
    static __device__ __forceinline__ long image(const Args&, long b) { return b; }
    static __device__ __forceinline__ vbtask::Span span(const Args& a, long img) {
        return vbtask::span(a.offsets[img], a.offsets[img + 1], a.total_rows, a.mean_rows != nullptr,
                            a.mean_rows != nullptr ? a.mean_rows[img] : 0, a.max_regions);
    }
};

// the clamped span of output sample b
template <typename Args>
__device__ __forceinline__ vbtask::Span sample_span(const Args& a, long b) {
    return Source<Args>::span(a, Source<Args>::image(a, b));
}

// Fine-tuning builder; of Args only the fields vbd_task_batch, vbw_task_batch and vbr_store_batch share are read (feat /
// out_feat by address), the sample's rows only through sample_span. A sample that owns nothing (kept == 0) is zeros, row 0 too.
// blockIdx.z == 0: the packed rows of a sample, once: row i goes to output row i + 1 while it is kept and into the column sum
// while i < count; the sum runs in row order, one __fadd_rn per row (np.sum(x, axis=0) of a C-contiguous fp32 array), and is
// divided in fp32 by (float)count (numpy: float32 array / Python int); count == 0: zeros.
// blockIdx.z == 1: the zero rows kept_b .. R - 1 (stores only, nothing to wait for).
template <typename In, typename Out, typename Args>
__global__ __launch_bounds__(Cols<In>::TASK_THREADS) void task_feat_kernel(const Args a) {
    typedef Cols<In> G;
    constexpr int ROWS = G::TASK_ROWS;
    const int F = a.feat_dim;
    const long c = ((long)blockIdx.x * G::TASK_THREADS + threadIdx.x) * G::N;
    if (c >= F) return;
    const long R = a.max_regions;
    for (long b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const vbtask::Span sp = sample_span(a, b);
        Out* const o = reinterpret_cast<Out*>(a.out_feat);
        const long dst = (b * R) * F + c;
        if (blockIdx.z == 1) {
            for (long r = sp.kept; r < R; ++r) G::store(o + (dst + r * F), typename G::Wide{});
            continue;
        }
        const In* src = reinterpret_cast<const In*>(a.feat) + sp.start * F + c;
        const long copied = sp.kept - 1;                       // packed rows 0 .. copied - 1 are output rows 1 .. copied
        const long lim = sp.mean > copied ? sp.mean : copied;  // <= sp.rows: nothing beyond the sample's span is read
        typename G::Wide s = {};
        for (long i0 = 0; i0 < lim; i0 += ROWS) {
            typename G::Raw h[ROWS];
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                h[u] = typename G::Raw{};
                if (i0 + u < lim) h[u] = *reinterpret_cast<const typename G::Raw*>(src + (i0 + u) * F);
            }
#pragma unroll
            for (int u = 0; u < ROWS; ++u) {
                const long i = i0 + u;
                const typename G::Wide v = G::widen(h[u]);
                if (i < copied) G::store(o + (dst + (i + 1) * F), v);
                if (i < sp.mean) {
#pragma unroll
                    for (int e = 0; e < G::N; ++e) s[e] = __fadd_rn(s[e], v[e]);
                }
            }
        }
        typename G::Wide g = {};
        if (sp.mean > 0) {
            const float n = (float)sp.mean;
#pragma unroll
            for (int e = 0; e < G::N; ++e) g[e] = __fdiv_rn(s[e], n);
        }
        G::store(o + dst, g);
    }
}

}  // namespace vbfeat
