// y = widen(x) for a flat binary16 array (include/vilbert_hip_wire.h: vbw_widen_f16) - the region targets of a float16 wire,
// whose rows are no 16-byte multiples. The batch-finishing calls of that header sit next to their fp32 siblings (batch.hip,
// task_batch.hip) and share the feature kernels of feat_rows.h, whose binary16 column group this kernel loads and stores with.
#include "feat_rows.h"
#include "../../include/vilbert_hip_wire.h"

namespace {

typedef vbfeat::Cols<_Float16> H;

constexpr int WW_THREADS = 256;
constexpr int64_t WW_MAX_BLOCKS = 1L << 20;

// y[i] = widen(x[i]): groups of 8 with one 16-byte load and two 16-byte stores, grid-strided; the n % 8 elements behind the
// last group one by one, by the first threads of block 0.
__global__ __launch_bounds__(WW_THREADS) void widen_f16_kernel(long groups, int tail, const uint16_t* __restrict__ x,
                                                               float* __restrict__ y) {
    for (long g = (long)blockIdx.x * WW_THREADS + threadIdx.x; g < groups; g += (long)gridDim.x * WW_THREADS)
        H::store(y + g * 8, H::widen(*reinterpret_cast<const H::Raw*>(x + g * 8)));
    if (blockIdx.x == 0 && (int)threadIdx.x < tail) {
        const long i = groups * 8 + threadIdx.x;
        y[i] = (float)__builtin_bit_cast(_Float16, x[i]);
    }
}

}  // namespace

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
