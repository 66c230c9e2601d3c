// Deterministic mode (vb_set_deterministic): the kernels that would add partial results with fp32 atomics - whose
// result depends on the order the blocks happen to finish in - store their partials to a workspace registered by the
// caller and a second kernel adds them in a fixed order: bit-identical results from run to run.
//
// One workspace PER DEVICE (a process may drive several GPUs: nn.DataParallel replicas, the reference's non-distributed
// multi-GPU path train_concap.py:513-515): a launch only ever uses the workspace registered for the device it runs on, and
// falls back to the fp32-atomics form when there is none. Each workspace is cut into DET_SLICES equal slices; every
// (device, stream) that issues such launches gets its own (first come, first served, for the lifetime of that
// registration), so the text / image / weight-gradient side streams keep overlapping. A stream that comes after the
// slices are taken, or a launch whose partials do not fit a slice, runs with atomics (correct, just not bit-reproducible)
// and is counted (vb_deterministic_fallbacks) - it is never an error.
#include "det_workspace.h"

#include <mutex>

#include "common.h"

namespace {

constexpr int DET_SLICES = 8;
constexpr int DET_MAX_DEV = 16;
struct DetDevice {
    float* ws = nullptr;
    size_t bytes = 0;
    hipStream_t streams[DET_SLICES];
    int nstreams = 0;
};
int g_det = 0;
DetDevice g_det_dev[DET_MAX_DEV];
long g_det_fallbacks = 0;
std::mutex g_det_mutex;     // autograd runs backward nodes on its own threads

}  // namespace

namespace vbdet {

bool det_on() { return g_det != 0; }

float* det_slice(hipStream_t st, size_t* slice_bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= DET_MAX_DEV) return nullptr;
    std::lock_guard<std::mutex> lock(g_det_mutex);
    DetDevice& d = g_det_dev[dev];
    if (d.ws == nullptr) return nullptr;
    const size_t slice = d.bytes / DET_SLICES / 16 * 16;
    *slice_bytes = slice;
    int k = -1;
    for (int i = 0; i < d.nstreams; ++i)
        if (d.streams[i] == st) { k = i; break; }
    if (k < 0) {
        if (d.nstreams == DET_SLICES) return nullptr;
        d.streams[d.nstreams] = st;
        k = d.nstreams++;
    }
    return d.ws + (size_t)k * (slice / sizeof(float));
}

void det_fallback() {
    std::lock_guard<std::mutex> lock(g_det_mutex);
    ++g_det_fallbacks;
}

float* det_claim(hipStream_t st, size_t need_bytes) {
    size_t slice = 0;
    float* base = det_slice(st, &slice);
    if (base != nullptr && need_bytes <= slice) return base;
    det_fallback();
    return nullptr;
}

}  // namespace vbdet

extern "C" int vb_set_deterministic(int on, void* workspace, int64_t workspace_bytes) {
    const int prev = g_det > 0 ? 1 : 0;
    if (on != 0 && on != 1) return prev;
    if (on && (workspace == nullptr || workspace_bytes <= 0 || !vb_aligned16(workspace))) return VB_E_BADARG;
    int dev = -1;
    if (on) {
        // the workspace serves the device it lives on, whichever device is current now
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, workspace) != hipSuccess) { (void)hipGetLastError(); return VB_E_BADARG; }
        dev = attr.device;
        if (dev < 0 || dev >= DET_MAX_DEV) return VB_E_BADARG;
    }
    std::lock_guard<std::mutex> lock(g_det_mutex);
    if (!on) {
        for (DetDevice& d : g_det_dev) d = DetDevice();
        g_det = 0;
        return prev;
    }
    DetDevice& d = g_det_dev[dev];
    // re-registering the same buffer keeps the stream -> slice assignment (captured graphs have it baked in)
    if (d.ws != static_cast<float*>(workspace) || d.bytes != (size_t)workspace_bytes) {
        d = DetDevice();
        d.ws = static_cast<float*>(workspace);
        d.bytes = (size_t)workspace_bytes;
    }
    g_det = 1;
    g_det_fallbacks = 0;
    return prev;
}

extern "C" int64_t vb_deterministic_fallbacks(void) {
    std::lock_guard<std::mutex> lock(g_det_mutex);
    return (int64_t)g_det_fallbacks;
}
