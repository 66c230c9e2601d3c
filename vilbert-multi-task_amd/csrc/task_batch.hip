// Device-side building of a fine-tuning batch from PACKED region data (include/vilbert_hip_task_inputs.h). The reference does
// this per sample on the host in numpy (vilbert/datasets/_image_features_reader.py:144-176: mean-region row and 5-number boxes;
// vqa_dataset.py:275-310 and refer_expression_dataset.py:241-296: float64 zero padding to max_region_num, mask, dense answer
// target, region IoU target) and the collate stacks the padded samples. Here the regions of all samples travel back to back and
// one pass writes the padded [B, R, F] block: the packed rows are read once, the output is written once.
// HBM-bound: 4 F (N + B R) bytes from fp32 rows. From binary16 rows (include/vilbert_hip_wire.h) a row is widened as it is read
// and the block is written as fp32 or bf16: 2 F bytes read per packed row, 4 F or 2 F written per output row. The feature kernel
// and its arithmetic are in feat_rows.h, one body for all three (input, output) kinds; the boxes / mask / IoU-target kernel and
// the launch pair are in task_meta.h, shared with the device-resident store (region_store.hip). The numpy restatement
// tests/task_batch_restatement.py pins every bit of every kernel, so each fp32 operation is an explicit round-to-nearest
// intrinsic: hipcc would contract a * b + c into an FMA, numpy and torch do not.
#include "task_meta.h"
#include "../../include/vilbert_hip_task_inputs.h"
#include "../../include/vilbert_hip_wire.h"

#pragma clang fp contract(off)

namespace {

using vbmeta::launch;

constexpr long DT_MAX_BLOCKS = 1L << 20;

// One block per (row, 256-column chunk), grid-strided; a thread owns one column and scans the K labels of its row in order, so
// the LAST matching k wins. The labels and scores of a row are block-uniform reads that stay in cache.
__global__ __launch_bounds__(256) void dense_target_kernel(long rows, int num_labels, int K, const int32_t* __restrict__ labels,
                                                           const float* __restrict__ scores, float* __restrict__ target, long ldt) {
    const long chunks = ((long)num_labels + 255) / 256;
    const long items = rows * chunks;
    for (long it = blockIdx.x; it < items; it += gridDim.x) {
        const long r = it / chunks;
        const long c = (it - r * chunks) * 256 + threadIdx.x;
        if (c >= num_labels) continue;
        const int32_t* lab = labels + r * K;
        const float* sc = scores + r * K;
        float v = 0.f;
        for (int k = 0; k < K; ++k)
            if ((long)lab[k] == c) v = sc[k];
        target[r * ldt + c] = v;
    }
}

// What both builders refuse alike (Args: vbd_task_batch or vbw_task_batch; vbfeat::Cols<In> names the input rows): the
// documented errors of the two calls but out_kind, in their documented order. The output extent is checked for fp32 elements
// whichever kind is written.
template <typename In, typename Args>
int check_args(const Args* a) {
    if (a == nullptr || a->batch < 0 || a->total_rows < 0 || a->max_regions <= 0 || a->feat_dim <= 0) return VB_E_BADARG;
    if (!(a->iou_floor >= 0.f)) return VB_E_BADARG;          // NaN too
    if (!a->feat || !a->boxes || !a->offsets || !a->image_wh || !a->out_feat || !a->out_spatials || !a->out_mask)
        return VB_E_BADARG;
    if ((a->ref_box == nullptr) != (a->out_iou == nullptr)) return VB_E_BADARG;
    if (a->feat_dim % vbfeat::Cols<In>::N != 0 || !vb_aligned16(a->feat) || !vb_aligned16(a->out_feat)) return VB_E_ALIGN;
    if (!vb_byte_extent_ok(a->total_rows, a->feat_dim, sizeof(In)) ||
        !vb_byte_extent_ok((int64_t)a->batch * a->max_regions, a->feat_dim, 4))
        return VB_E_RANGE;
    return 0;
}

}  // namespace

extern "C" int vbd_task_finish_batch(void* stream, const vbd_task_batch* a) {
    if (const int e = check_args<float>(a)) return e;
    return launch<float, float>((hipStream_t)stream, *a);
}

extern "C" int vbw_task_finish_batch(void* stream, const vbw_task_batch* a) {
    if (a != nullptr && a->out_kind != VBW_OUT_F32 && a->out_kind != VBW_OUT_BF16) return VB_E_BADARG;
    if (const int e = check_args<_Float16>(a)) return e;
    return a->out_kind == VBW_OUT_BF16 ? launch<_Float16, vbfeat::bf16>((hipStream_t)stream, *a)
                                       : launch<_Float16, float>((hipStream_t)stream, *a);
}

extern "C" int vbd_dense_target(void* stream, int64_t rows, int32_t num_labels, int32_t K, const int32_t* labels,
                                const float* scores, float* target, int64_t ldt) {
    if (rows < 0 || num_labels <= 0 || K <= 0 || ldt < num_labels) return VB_E_BADARG;
    if (!labels || !scores || !target) return VB_E_BADARG;
    if (!vb_byte_extent_ok(rows, ldt, 4) || !vb_byte_extent_ok(rows, K, 4)) return VB_E_RANGE;
    if (rows == 0) return 0;
    const int64_t items = rows * (((int64_t)num_labels + 255) / 256);
    hipLaunchKernelGGL(dense_target_kernel, dim3((unsigned)(items < DT_MAX_BLOCKS ? items : DT_MAX_BLOCKS)), dim3(256), 0,
                       (hipStream_t)stream, (long)rows, (int)num_labels, (int)K, labels, scores, target, (long)ldt);
    VB_LAUNCH_CHECK();
    return 0;
}
