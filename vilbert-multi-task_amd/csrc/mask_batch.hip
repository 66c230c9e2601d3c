// Device-side MLM and region masking of a pre-training batch (include/vilbert_hip_inputs.h): the choice the reference makes per
// sample in Python inside its workers (vilbert/datasets/concept_cap_dataset.py:608-670, random_word / random_region) drawn from
// the counter-based hash of rng.h instead, so a source that keeps unmasked samples gets a fresh mask per pass without going
// back through the host. Same per-site rule and probabilities; not the reference's `random` stream.
// The numpy restatement tests/masking_restatement.py pins every bit of both kernels.
#include "common.h"
#include "rng.h"
#include "../../include/vilbert_hip_inputs.h"

namespace {

constexpr int MB_WAVE = 64;            // one wave per sample: T and R are a few dozen
constexpr int ZR_THREADS = 256;
constexpr long ZR_MAX_BLOCKS = 2048;   // 8 blocks per CU, the rows beyond that are grid-strided

__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float uniform24(uint32_t h) { return (float)(h >> 8) * (1.0f / 16777216.0f); }

// out_input_ids may alias input_ids (a position is read and written by the same lane): no __restrict__ on the id pointers.
__global__ __launch_bounds__(MB_WAVE) void concap_mask_kernel(const vbi_mask_args a) {
    const long b = blockIdx.x;
    const int lane = threadIdx.x;
    const int T = a.tokens, R = a.regions;
    const uint64_t L = (uint64_t)(T > R ? T : R);
    const uint64_t base_idx = (uint64_t)b * 3u * L;          // stream s of sample b starts at base_idx + s * L
    const float p = a.p_select;

    long long len = 0, boxes = 0;
    for (int t = lane; t < T; t += MB_WAVE) len += a.input_mask[b * T + t];
    for (int r = lane; r < R; r += MB_WAVE) boxes += a.image_mask[b * R + r];
    len = wave_sum_i64(len);
    boxes = wave_sum_i64(boxes);

    for (int t = lane; t < T; t += MB_WAVE) {
        const int64_t id = a.input_ids[b * T + t];
        int64_t out = id, label = -1;
        if (t >= 1 && t <= len - 2) {
            const float u = uniform24(vb_hash(a.seed, base_idx + (uint64_t)t));
            if (u < p) {
                const float v = u / p;
                if (v < 0.8f)
                    out = a.mask_token_id;
                else if (v < 0.9f)
                    out = (int64_t)(((uint64_t)vb_hash(a.seed, base_idx + L + (uint64_t)t) * (uint64_t)a.vocab_size) >> 32);
                label = id;
            }
        }
        a.out_input_ids[b * T + t] = out;
        a.lm_label_ids[b * T + t] = label;
    }

    // regions, 64 at a time: the lanes draw for regions chunk .. chunk + 63, the ballot of the selected ones is wave-uniform, and
    // lane j then ORs the overlap rows of just those regions into its own columns (no LDS, no atomics). A column beyond the
    // first chunk re-reads what the SAME lane stored for it.
    const float* ov = a.overlaps + b * R * (long)R;
    for (int chunk = 0; chunk < R; chunk += MB_WAVE) {
        const int i = chunk + lane;
        bool sel = false, zero = false;
        if (i < R) {
            if (i < boxes) {
                const float u = uniform24(vb_hash(a.seed, base_idx + 2u * L + (uint64_t)i));
                if (u < p) {
                    sel = true;
                    zero = u / p < 0.9f;
                }
            }
            a.image_label[b * R + i] = sel ? 1 : -1;
            a.zero_row[b * R + i] = zero ? 1 : 0;
        }
        const unsigned long long chosen = __ballot(sel);
        for (int j = lane; j < R; j += MB_WAVE) {
            int64_t m = chunk == 0 ? 0 : a.masked_label[b * R + j];
            for (unsigned long long rest = chosen; rest != 0; rest &= rest - 1) {
                const int k = __ffsll(rest) - 1;
                if (ov[(long)(chunk + k) * R + j] > 0.4f) m = 1;
            }
            a.masked_label[b * R + j] = m;
        }
    }
}

// One block per row (grid-strided), one 16-byte chunk per thread and step. COPY: every row of `out` is written (zeros or the row
// of x, which is not read where it is flagged); in place: only the flagged rows of x are touched. HBM-bound; at the feature
// width of the models (2048 floats = 512 chunks) a thread has two independent loads in flight per row and 8 blocks share a CU.
template <bool COPY>
__global__ __launch_bounds__(ZR_THREADS) void zero_rows_kernel(long rows, int chunks, float* x, long ldx,
                                                               const uint8_t* __restrict__ flags, float* out, long ldo) {
    for (long r = blockIdx.x; r < rows; r += gridDim.x) {
        const bool z = flags[r] != 0;          // block-uniform
        if (!COPY && !z) continue;
        const float* src = x + r * ldx;
        float* dst = COPY ? out + r * ldo : x + r * ldx;
#pragma unroll 2
        for (int c = threadIdx.x; c < chunks; c += ZR_THREADS) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (COPY && !z) v = *reinterpret_cast<const f32x4*>(src + 4 * (long)c);
            *reinterpret_cast<f32x4*>(dst + 4 * (long)c) = v;
        }
    }
}

}  // namespace

extern "C" int vbi_concap_mask_batch(void* stream, const vbi_mask_args* a) {
    if (a == nullptr || a->batch < 0 || a->tokens <= 0 || a->regions <= 0 || a->vocab_size <= 0) return VB_E_BADARG;
    if (a->mask_token_id < 0 || a->mask_token_id >= a->vocab_size) return VB_E_BADARG;
    if (!(a->p_select >= 0.f && a->p_select <= 1.f)) return VB_E_BADARG;          // NaN too
    if (!a->input_ids || !a->input_mask || !a->image_mask || !a->overlaps || !a->out_input_ids || !a->lm_label_ids ||
        !a->image_label || !a->masked_label || !a->zero_row)
        return VB_E_BADARG;
    if (!vb_byte_extent_ok((int64_t)a->batch * a->regions, a->regions, 4)) return VB_E_RANGE;
    if (a->batch == 0) return 0;
    hipLaunchKernelGGL(concap_mask_kernel, dim3((unsigned)a->batch), dim3(MB_WAVE), 0, (hipStream_t)stream, *a);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbi_zero_rows(void* stream, int64_t rows, int32_t n, float* x, int64_t ldx, const uint8_t* flags, float* out,
                             int64_t ldo) {
    if (rows < 0 || n <= 0 || ldx < n || (out != nullptr && ldo < n)) return VB_E_BADARG;
    if (!x || !flags || out == x) return VB_E_BADARG;
    if (n % 4 != 0 || !vb_row32_ok(x, ldx) || (out != nullptr && !vb_row32_ok(out, ldo))) return VB_E_ALIGN;
    if (!vb_byte_extent_ok(rows, ldx, 4) || (out != nullptr && !vb_byte_extent_ok(rows, ldo, 4))) return VB_E_RANGE;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(rows < ZR_MAX_BLOCKS ? rows : ZR_MAX_BLOCKS));
    if (out != nullptr)
        hipLaunchKernelGGL(zero_rows_kernel<true>, grid, dim3(ZR_THREADS), 0, st, (long)rows, n / 4, x, (long)ldx, flags, out,
                           (long)ldo);
    else
        hipLaunchKernelGGL(zero_rows_kernel<false>, grid, dim3(ZR_THREADS), 0, st, (long)rows, n / 4, x, (long)ldx, flags,
                           (float*)nullptr, 0L);
    VB_LAUNCH_CHECK();
    return 0;
}
