// Fine-tuning batches from a DEVICE-RESIDENT region store (include/vilbert_hip_store.h): the detector's regions of a whole
// dataset stay on the device and a batch is named by one image index per sample, so a step sends a few hundred bytes of ids
// where the packed builders (task_batch.hip) are sent every feature row. No kernel of its own: the feature kernel of
// feat_rows.h and the boxes / mask / IoU-target kernel of task_meta.h are instantiated here for vbr_store_batch, whose
// vbfeat::Source names a sample's image by its validated id word (store_rows.h) where a packed batch names it by b. The
// arithmetic after that is the packed builders', bit for bit (tests/test_region_store_gpu.py).
// HBM-bound like them: the row offsets of a store pass 2^31 elements from row 2^20 on (F = 2048), and every element offset in
// the two kernels is formed in 64 bits.
#include "task_meta.h"
#include "store_rows.h"
#include "../../include/vilbert_hip_store.h"

#pragma clang fp contract(off)

namespace vbfeat {

// Output sample b shows image image_ids[b]: image() validates the id (block-uniform, read once per sample) and an invalid
// one reads no store word at all; span() clamps the words of a valid one.
template <>
struct Source<vbr_store_batch> {
    static __device__ __forceinline__ long image(const vbr_store_batch& a, long b) {
        return vbstore::image(a.image_ids[b], a.num_images);
    }
    static __device__ __forceinline__ vbtask::Span span(const vbr_store_batch& a, long img) {
        return vbstore::span(img, a.image_offsets, a.mean_rows != nullptr, a.mean_rows, a.total_rows, a.max_regions);
    }
};

}  // namespace vbfeat

namespace {

// the documented errors of the call, in their documented order
int check_args(const vbr_store_batch* a) {
    if (a == nullptr || a->batch < 0 || a->total_rows < 0 || a->num_images < 0 || a->max_regions <= 0 || a->feat_dim <= 0)
        return VB_E_BADARG;
    if (!(a->iou_floor >= 0.f)) return VB_E_BADARG;          // NaN too
    if ((a->feat_kind != VBR_FEAT_F32 && a->feat_kind != VBR_FEAT_F16) || (a->out_kind != VBR_OUT_F32 && a->out_kind != VBR_OUT_BF16))
        return VB_E_BADARG;
    if (a->out_kind == VBR_OUT_BF16 && a->feat_kind == VBR_FEAT_F32) return VB_E_BADARG;
    if (!a->feat || !a->boxes || !a->image_offsets || !a->image_wh || !a->image_ids || !a->out_feat || !a->out_spatials ||
        !a->out_mask)
        return VB_E_BADARG;
    if ((a->ref_box == nullptr) != (a->out_iou == nullptr)) return VB_E_BADARG;
    const bool half = a->feat_kind == VBR_FEAT_F16;
    const int group = half ? vbfeat::Cols<_Float16>::N : vbfeat::Cols<float>::N;
    if (a->feat_dim % group != 0 || !vb_aligned16(a->feat) || !vb_aligned16(a->out_feat)) return VB_E_ALIGN;
    if (!vb_byte_extent_ok(a->total_rows, a->feat_dim, half ? 2 : 4) ||
        !vb_byte_extent_ok((int64_t)a->batch * a->max_regions, a->feat_dim, 4))
        return VB_E_RANGE;
    return 0;
}

}  // namespace

extern "C" int vbr_store_finish_batch(void* stream, const vbr_store_batch* a) {
    if (const int e = check_args(a)) return e;
    const hipStream_t st = (hipStream_t)stream;
    if (a->feat_kind == VBR_FEAT_F32) return vbmeta::launch<float, float>(st, *a);
    return a->out_kind == VBR_OUT_BF16 ? vbmeta::launch<_Float16, vbfeat::bf16>(st, *a)
                                       : vbmeta::launch<_Float16, float>(st, *a);
}
