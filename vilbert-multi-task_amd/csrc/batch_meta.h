// The launches of a batch-finishing call that do not touch the feature block: boxes, masks, labels and the IoU target. The fp32
// calls (batch.hip, task_batch.hip) and the binary16 calls (wire16.hip) enqueue the SAME kernels through these two functions, so
// there is one copy of that arithmetic. Arguments are checked by the callers; the feature pointers of the structs are not read.
#pragma once
#include "common.h"
#include "../../include/vilbert_hip_task_inputs.h"

namespace vbmeta {
// batch.hip: boxes, region mask and the objective-1 label edit of a Conceptual-Captions batch; 0 or a hipError_t
int concap_meta(hipStream_t st, const vb_concap_batch& a);
// task_batch.hip: spatials, region mask and the optional IoU target of a fine-tuning batch (batch > 0); 0 or a hipError_t
int task_meta(hipStream_t st, const vbd_task_batch& a);
}  // namespace vbmeta
