// The boxes / mask / IoU-target kernel of the fine-tuning batch builders and the launch pair they share: task_batch.hip (packed
// regions: vbd_task_batch, vbw_task_batch) and region_store.hip (a device-resident store: vbr_store_batch). ONE body: which
// rows and which per-image words a sample reads is decided by vbfeat::Source<Args> (feat_rows.h), everything after that is the
// same arithmetic - stated in include/vilbert_hip_task_inputs.h, restated in numpy by tests/task_batch_restatement.py, so each
// fp32 operation is an explicit round-to-nearest intrinsic: hipcc would contract a * b + c into an FMA, numpy does not.
#pragma once
#include "feat_rows.h"

#pragma clang fp contract(off)

namespace vbmeta {

constexpr int TM_THREADS = 256;
constexpr unsigned GRID_Y_MAX = 65535;

// the reference's iou() for one anchor against one box (refer_expression_dataset.py:19-56, the + 1 pixel convention)
__device__ __forceinline__ float iou_px(float ax1, float ay1, float ax2, float ay2, float gx1, float gy1, float gx2, float gy2) {
    const float g_area = __fmul_rn(__fadd_rn(__fsub_rn(gx2, gx1), 1.f), __fadd_rn(__fsub_rn(gy2, gy1), 1.f));
    const float a_area = __fmul_rn(__fadd_rn(__fsub_rn(ax2, ax1), 1.f), __fadd_rn(__fsub_rn(ay2, ay1), 1.f));
    float iw = __fadd_rn(__fsub_rn(fminf(ax2, gx2), fmaxf(ax1, gx1)), 1.f);
    float ih = __fadd_rn(__fsub_rn(fminf(ay2, gy2), fmaxf(ay1, gy1)), 1.f);
    if (iw < 0.f) iw = 0.f;
    if (ih < 0.f) ih = 0.f;
    const float inter = __fmul_rn(iw, ih);
    return __fdiv_rn(inter, __fsub_rn(__fadd_rn(a_area, g_area), inter));
}

// One block per sample: boxes, region mask and (optional) the region-IoU target; a thread owns output row r. The feature
// pointers of Args are not read. The sample's image (block-uniform) is looked up once: its span and its size come from it; a
// sample without an image (img < 0) keeps no row, so its size is never used and never read.
template <typename Args>
__global__ __launch_bounds__(TM_THREADS) void task_meta_kernel(const Args a) {
    const long R = a.max_regions;
    for (long b = blockIdx.x; b < a.batch; b += gridDim.x) {
        const long img = vbfeat::Source<Args>::image(a, b);
        const vbtask::Span sp = vbfeat::Source<Args>::span(a, img);
        int32_t W = 0, H = 0;
        if (img >= 0) {
            W = a.image_wh[2 * img];
            H = a.image_wh[2 * img + 1];
        }
        const float w = (float)W, h = (float)H, wh = (float)((int64_t)W * (int64_t)H);
        float gx1 = 0.f, gy1 = 0.f, gx2 = 0.f, gy2 = 0.f;
        if (a.ref_box != nullptr) {
            gx1 = a.ref_box[4 * b]; gy1 = a.ref_box[4 * b + 1]; gx2 = a.ref_box[4 * b + 2]; gy2 = a.ref_box[4 * b + 3];
        }
        for (long r = threadIdx.x; r < R; r += TM_THREADS) {
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, t = 0.f;
            const bool kept = r < sp.kept;
            if (kept) {
                float x1 = 0.f, y1 = 0.f, x2 = w, y2 = h;          // the global row's pixel box
                if (r == 0) {
                    s2 = 1.f; s3 = 1.f; s4 = 1.f;
                } else {
                    const float* box = a.boxes + (sp.start + r - 1) * 4;
                    x1 = box[0]; y1 = box[1]; x2 = box[2]; y2 = box[3];
                    s0 = __fdiv_rn(x1, w);
                    s1 = __fdiv_rn(y1, h);
                    s2 = __fdiv_rn(x2, w);
                    s3 = __fdiv_rn(y2, h);
                    s4 = __fdiv_rn(__fmul_rn(__fsub_rn(y2, y1), __fsub_rn(x2, x1)), wh);
                }
                if (a.out_iou != nullptr) {
                    t = iou_px(x1, y1, x2, y2, gx1, gy1, gx2, gy2);
                    if (t < a.iou_floor) t = 0.f;
                }
            }
            float* sp_out = a.out_spatials + (b * R + r) * 5;
            sp_out[0] = s0; sp_out[1] = s1; sp_out[2] = s2; sp_out[3] = s3; sp_out[4] = s4;
            a.out_mask[b * R + r] = kept ? 1 : 0;
            if (a.out_iou != nullptr) a.out_iou[b * R + r] = t;
        }
    }
}

// the feature kernel of (In, Out), then the boxes / mask / IoU target; arguments checked by the callers
template <typename In, typename Out, typename Args>
int launch(hipStream_t st, const Args& a) {
    typedef vbfeat::Cols<In> G;
    if (a.batch == 0) return 0;
    const unsigned by = (unsigned)a.batch < GRID_Y_MAX ? (unsigned)a.batch : GRID_Y_MAX;
    const dim3 grid((unsigned)((a.feat_dim / G::N + G::TASK_THREADS - 1) / G::TASK_THREADS), by, 2);
    hipLaunchKernelGGL((vbfeat::task_feat_kernel<In, Out, Args>), grid, dim3(G::TASK_THREADS), 0, st, a);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(task_meta_kernel<Args>, dim3((unsigned)a.batch), dim3(TM_THREADS), 0, st, a);
    VB_LAUNCH_CHECK();
    return 0;
}

}  // namespace vbmeta
