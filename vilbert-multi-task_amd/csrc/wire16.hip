// Batch finishing from binary16 region features (include/vilbert_hip_wire.h): the arithmetic of batch.hip's and task_batch.hip's
// feature kernels on rows that are widened to fp32 as they are read, with an fp32 or a bf16 feature output. A feature store that
// keeps the detector's activations as float16 sends half the bytes over the bus; the bf16 stream rounds the feature block to
// bf16 before its first GEMM anyway, so with out_kind = 1 the fp32 block and the cast launch are never made.
// HBM-bound: per row of F columns 2 F bytes are read and 4 F (fp32) or 2 F (bf16) written - 25 % / 50 % below the fp32 kernels.
// A thread owns 8 feature columns: one 16-byte load per row, two 16-byte stores (fp32) or one (bf16). The kernels are held bit
// for bit to the fp32 calls on the widened arrays (tests/test_wire16_gpu.py), so each fp32 operation is an explicit
// round-to-nearest intrinsic and nothing is contracted.
#include "common.h"
#include "task_rows.h"
#include "batch_meta.h"
#include "../../include/vilbert_hip_wire.h"

#pragma clang fp contract(off)

namespace {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int WF_THREADS = 64;          // one wave owns 512 feature columns of one sample: 4 blocks per sample at F = 2048
constexpr int WF_UNROLL = 8;            // independent 16-byte loads a thread has in flight
constexpr int WW_THREADS = 256;
constexpr unsigned GRID_Y_MAX = 65535;
constexpr int64_t WW_MAX_BLOCKS = 1L << 20;

// binary16 -> fp32 is exact (v_cvt_f32_f16; the kernels run with denormals on: subnormals keep their value)
__device__ __forceinline__ f32x8 widen8(f16x8 h) { return __builtin_convertvector(h, f32x8); }

__device__ __forceinline__ f16x8 zero_h8() {
    const f16x8 z = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f,
                     (_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    return z;
}

// 8 columns of one output row, from element `elem` of `out` (counted in elements of the output type; a multiple of 8)
template <bool BF16>
__device__ __forceinline__ void store8(void* out, long elem, f32x8 v) {
    if constexpr (BF16) {
        u32x4 w;
        w[0] = vb_bf16_pack(v[0], v[1]);
        w[1] = vb_bf16_pack(v[2], v[3]);
        w[2] = vb_bf16_pack(v[4], v[5]);
        w[3] = vb_bf16_pack(v[6], v[7]);
        *reinterpret_cast<u32x4*>(static_cast<uint16_t*>(out) + elem) = w;
    } else {
        float* p = static_cast<float*>(out) + elem;
        const f32x4 lo = {v[0], v[1], v[2], v[3]}, hi = {v[4], v[5], v[6], v[7]};
        *reinterpret_cast<f32x4*>(p) = lo;
        *reinterpret_cast<f32x4*>(p + 4) = hi;
    }
}

__device__ __forceinline__ f32x8 zero_f8() {
    const f32x8 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    return z;
}

// One thread owns 8 feature columns of one sample: out[b, r + 1, c] = x[b, r, c], out[b, 0, c] = sum_r x / count, where
// x[b, r] is the widened row, or zeros where zero_row flags it (such a row is not loaded). The sum runs over r = 0 .. R - 1 in
// fp32 in that order, one __fadd_rn per row - a flagged row adds its +0, as the cleared fp32 row does - and the division is
// done in fp64 and rounded to fp32 (batch.hip). The loads of WF_UNROLL rows are issued before the first of them is used.
template <bool BF16>
__global__ __launch_bounds__(WF_THREADS) void concap_feat16_kernel(int B, int R, int F, const uint16_t* __restrict__ in,
                                                                   const int64_t* __restrict__ masked_label,
                                                                   const uint8_t* __restrict__ zero_row, void* __restrict__ out) {
    const long c = ((long)blockIdx.x * WF_THREADS + threadIdx.x) * 8;
    if (c >= F) return;
    for (long b = blockIdx.y; b < B; b += gridDim.y) {
        int cnt = 0;
        for (int r = 0; r < R; ++r) cnt += masked_label[b * R + r] == 0 ? 1 : 0;
        if (cnt == 0) cnt = 1;
        const uint16_t* src = in + b * R * F + c;
        const uint8_t* flags = zero_row != nullptr ? zero_row + b * R : nullptr;
        const long dst = b * (R + 1) * F + c;
        f32x8 s = zero_f8();
        for (int r0 = 0; r0 < R; r0 += WF_UNROLL) {
            f16x8 h[WF_UNROLL];
#pragma unroll
            for (int u = 0; u < WF_UNROLL; ++u) {
                h[u] = zero_h8();
                const int r = r0 + u;
                if (r < R && (flags == nullptr || flags[r] == 0)) h[u] = *reinterpret_cast<const f16x8*>(src + (long)r * F);
            }
#pragma unroll
            for (int u = 0; u < WF_UNROLL; ++u) {
                const int r = r0 + u;
                if (r < R) {
                    const f32x8 v = widen8(h[u]);
                    store8<BF16>(out, dst + (long)(r + 1) * F, v);
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[e] = __fadd_rn(s[e], v[e]);
                }
            }
        }
        f32x8 g;
#pragma unroll
        for (int e = 0; e < 8; ++e) g[e] = (float)((double)s[e] / (double)cnt);
        store8<BF16>(out, dst, g);
    }
}

__device__ __forceinline__ vbtask::Span sample_span(const vbw_task_batch& a, long b) {
    return vbtask::span(a.offsets[b], a.offsets[b + 1], a.total_rows, a.mean_rows != nullptr,
                        a.mean_rows != nullptr ? a.mean_rows[b] : 0, a.max_regions);
}

// task_batch.hip's feature kernel on binary16 rows, 8 columns per thread.
// blockIdx.z == 0: the packed rows of a sample, once: row i goes to output row i + 1 while it is kept and into the column sum
// while i < count; the sum runs in row order, one __fadd_rn per row, and is divided in fp32 by (float)count.
// blockIdx.z == 1: the zero rows kept_b .. R - 1 (stores only, nothing to wait for).
template <bool BF16>
__global__ __launch_bounds__(WF_THREADS) void task_feat16_kernel(const vbw_task_batch a) {
    const int F = a.feat_dim;
    const long c = ((long)blockIdx.x * WF_THREADS + threadIdx.x) * 8;
    if (c >= F) return;
    const long R = a.max_regions;
    for (long b = blockIdx.y; b < a.batch; b += gridDim.y) {
        const vbtask::Span sp = sample_span(a, b);
        const long dst = (b * R) * F + c;
        if (blockIdx.z == 1) {
            for (long r = sp.kept; r < R; ++r) store8<BF16>(a.out_feat, dst + r * F, zero_f8());
            continue;
        }
        const uint16_t* src = a.feat + sp.start * F + c;
        const long copied = sp.kept - 1;                       // packed rows 0 .. copied - 1 are output rows 1 .. copied
        const long lim = sp.mean > copied ? sp.mean : copied;  // <= sp.rows: nothing beyond the sample's span is read
        f32x8 s = zero_f8();
        for (long i0 = 0; i0 < lim; i0 += WF_UNROLL) {
            f16x8 h[WF_UNROLL];
#pragma unroll
            for (int u = 0; u < WF_UNROLL; ++u) {
                h[u] = zero_h8();
                if (i0 + u < lim) h[u] = *reinterpret_cast<const f16x8*>(src + (i0 + u) * F);
            }
#pragma unroll
            for (int u = 0; u < WF_UNROLL; ++u) {
                const long i = i0 + u;
                const f32x8 v = widen8(h[u]);
                if (i < copied) store8<BF16>(a.out_feat, dst + (i + 1) * F, v);
                if (i < sp.mean) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[e] = __fadd_rn(s[e], v[e]);
                }
            }
        }
        f32x8 g = zero_f8();
        if (sp.mean > 0) {
            const float n = (float)sp.mean;
#pragma unroll
            for (int e = 0; e < 8; ++e) g[e] = __fdiv_rn(s[e], n);
        }
        store8<BF16>(a.out_feat, dst, g);
    }
}

// y[i] = widen(x[i]): groups of 8 with one 16-byte load and two 16-byte stores, grid-strided; the n % 8 elements behind the
// last group one by one, by the first threads of block 0.
__global__ __launch_bounds__(WW_THREADS) void widen_f16_kernel(long groups, int tail, const uint16_t* __restrict__ x,
                                                               float* __restrict__ y) {
    for (long g = (long)blockIdx.x * WW_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * WW_THREADS)
        store8<false>(y, g * 8, widen8(*reinterpret_cast<const f16x8*>(x + g * 8)));
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const long i = groups * 8 + threadIdx.x;
        y[i] = (float)__builtin_bit_cast(_Float16, x[i]);
    }
}

// rows * ld elements of `bytes` bytes each whose BYTE offsets stay inside int64 (the kernels form pointers from them)
inline bool extent_ok(int64_t rows, int64_t ld, int64_t bytes) {
    return vb_extent_ok(rows, ld) && (rows <= 0 || rows * ld <= INT64_MAX / bytes);
}

}  // namespace

extern "C" int vbw_concap_finish_batch(void* stream, const vbw_concap_batch* a) {
    if (a == nullptr || a->batch < 0 || a->regions <= 0 || a->tokens <= 0 || a->feat_dim <= 0) return VB_E_BADARG;
    if (a->out_kind != VBW_OUT_F32 && a->out_kind != VBW_OUT_BF16) return VB_E_BADARG;
    if (!a->image_feat || !a->image_loc || !a->image_mask || !a->masked_label || !a->is_next || !a->image_label ||
        !a->lm_label_ids || !a->out_image_feat || !a->out_image_loc || !a->out_image_mask || !a->out_image_label ||
        !a->out_lm_label_ids)
        return VB_E_BADARG;
    if (a->feat_dim % 8 != 0 || !vb_aligned16(a->image_feat) || !vb_aligned16(a->out_image_feat)) return VB_E_ALIGN;
    if (!extent_ok((int64_t)a->batch * a->regions, a->feat_dim, 2) ||
        !extent_ok((int64_t)a->batch * ((int64_t)a->regions + 1), a->feat_dim, 4))
        return VB_E_RANGE;
    if (a->batch == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned by = (unsigned)a->batch < GRID_Y_MAX ? (unsigned)a->batch : GRID_Y_MAX;
    const dim3 grid((unsigned)((a->feat_dim / 8 + WF_THREADS - 1) / WF_THREADS), by);
    if (a->out_kind == VBW_OUT_BF16)
        hipLaunchKernelGGL(concap_feat16_kernel<true>, grid, dim3(WF_THREADS), 0, st, a->batch, a->regions, a->feat_dim,
                           a->image_feat, a->masked_label, a->zero_row, a->out_image_feat);
    else
        hipLaunchKernelGGL(concap_feat16_kernel<false>, grid, dim3(WF_THREADS), 0, st, a->batch, a->regions, a->feat_dim,
                           a->image_feat, a->masked_label, a->zero_row, a->out_image_feat);
    VB_LAUNCH_CHECK();
    vb_concap_batch m = {};                 // the feature pointers stay NULL: the meta kernel does not read them
    m.batch = a->batch; m.regions = a->regions; m.tokens = a->tokens; m.feat_dim = a->feat_dim; m.objective = a->objective;
    m.image_loc = a->image_loc; m.image_mask = a->image_mask; m.masked_label = a->masked_label; m.is_next = a->is_next;
    m.image_label = a->image_label; m.lm_label_ids = a->lm_label_ids;
    m.out_image_loc = a->out_image_loc; m.out_image_mask = a->out_image_mask; m.out_image_label = a->out_image_label;
    m.out_lm_label_ids = a->out_lm_label_ids;
    return vbmeta::concap_meta(st, m);
}

extern "C" int vbw_task_finish_batch(void* stream, const vbw_task_batch* a) {
    if (a == nullptr || a->batch < 0 || a->total_rows < 0 || a->max_regions <= 0 || a->feat_dim <= 0) return VB_E_BADARG;
    if (!(a->iou_floor >= 0.f)) return VB_E_BADARG;          // NaN too
    if (a->out_kind != VBW_OUT_F32 && a->out_kind != VBW_OUT_BF16) return VB_E_BADARG;
    if (!a->feat || !a->boxes || !a->offsets || !a->image_wh || !a->out_feat || !a->out_spatials || !a->out_mask)
        return VB_E_BADARG;
    if ((a->ref_box == nullptr) != (a->out_iou == nullptr)) return VB_E_BADARG;
    if (a->feat_dim % 8 != 0 || !vb_aligned16(a->feat) || !vb_aligned16(a->out_feat)) return VB_E_ALIGN;
    if (!extent_ok(a->total_rows, a->feat_dim, 2) || !extent_ok((int64_t)a->batch * a->max_regions, a->feat_dim, 4))
        return VB_E_RANGE;
    if (a->batch == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const unsigned by = (unsigned)a->batch < GRID_Y_MAX ? (unsigned)a->batch : GRID_Y_MAX;
    const dim3 grid((unsigned)((a->feat_dim / 8 + WF_THREADS - 1) / WF_THREADS), by, 2);
    if (a->out_kind == VBW_OUT_BF16)
        hipLaunchKernelGGL(task_feat16_kernel<true>, grid, dim3(WF_THREADS), 0, st, *a);
    else
        hipLaunchKernelGGL(task_feat16_kernel<false>, grid, dim3(WF_THREADS), 0, st, *a);
    VB_LAUNCH_CHECK();
    vbd_task_batch m = {};                  // feat / out_feat stay NULL: the meta kernel does not read them
    m.batch = a->batch; m.max_regions = a->max_regions; m.feat_dim = a->feat_dim; m.iou_floor = a->iou_floor;
    m.total_rows = a->total_rows; m.boxes = a->boxes; m.offsets = a->offsets; m.image_wh = a->image_wh;
    m.mean_rows = a->mean_rows; m.ref_box = a->ref_box; m.out_spatials = a->out_spatials; m.out_mask = a->out_mask;
    m.out_iou = a->out_iou;
    return vbmeta::task_meta(st, m);
}

extern "C" int vbw_widen_f16(void* stream, int64_t n, const uint16_t* x, float* y) {
    if (n < 0 || x == nullptr || y == nullptr) return VB_E_BADARG;
    if (!vb_aligned16(x) || !vb_aligned16(y)) return VB_E_ALIGN;
    if (n > INT64_MAX / 4) return VB_E_RANGE;
    if (n == 0) return 0;
    const int64_t groups = n / 8;
    hipLaunchKernelGGL(widen_f16_kernel, dim3(vb_grid_for(groups, WW_THREADS, WW_MAX_BLOCKS)), dim3(WW_THREADS), 0,
                       (hipStream_t)stream, (long)groups, (int)(n % 8), x, y);
    VB_LAUNCH_CHECK();
    return 0;
}
