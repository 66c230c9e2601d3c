// Deterministic workspace (det_workspace.hip, vb_set_deterministic): scratch for the kernels that replace fp32 atomics
// by partial results summed in a fixed order (split-K GEMMs, the skinny and bf16 weight gradients, the ordered
// text-embedding backward).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace vbdet {

bool det_on();   // the setting
// slice of (current device, stream) and its size, or nullptr: the device has no workspace or its slices are taken
float* det_slice(hipStream_t st, size_t* slice_bytes);
void det_fallback();   // counts a launch that ran with atomics although the setting is on (vb_deterministic_fallbacks)
// the slice of (current device, stream) if there is one and need_bytes fit it; otherwise counts one fallback -> nullptr
float* det_claim(hipStream_t st, size_t need_bytes);

}  // namespace vbdet
