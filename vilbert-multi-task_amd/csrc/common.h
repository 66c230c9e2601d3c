// Shared device helpers for the gfx950 kernels (wave = 64 lanes everywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_round.h"  // host-only part: the one fp32 -> bf16 rounding (NaN-safe) of every bf16 store
#include "gemm_plan.h"   // host-only part: the C ABI header, vb_aligned16, vb_env_int / vb_env_float
#include "row_checks.h"  // host-only part: extent / alignment checks and grid sizes of the row kernels

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define VB_LAUNCH_CHECK()                         \
    do {                                          \
        hipError_t e__ = hipGetLastError();       \
        if (e__ != hipSuccess) return (int)e__;   \
    } while (0)

// device pointer registered with vb_set_seed_epoch (or null): every dropout launch passes it to its kernel
const uint64_t* vb_seed_epoch();

namespace vbemb {
// vb_text_embed_bwd under the deterministic setting (embed_bwd.hip): 0 = the ordered kernels ran on the stream's
// workspace slice; -1 = the setting is off, or there is no slice / it is too small (counted by
// vb_deterministic_fallbacks) - the caller runs the atomic kernels; > 0 = launch error (hipError_t)
int text_embed_bwd_det(hipStream_t st, int batch, int n_tok, int hidden, int vocab, int n_types, int n_tasks,
                       const int64_t* ids, const int64_t* seg, const int64_t* task_ids, const float* dx, float* dword,
                       float* dpos, float* dtype, float* dtask, bool skip_pos0 = false, bool skip_type0 = false);
// the body of vb_text_embed_bwd (embed.hip): argument checks, the ordered reduction above or the atomic kernels. skip_pos0 /
// skip_type0 (vbb_text_embed_bwd, the baseline's padding_idx = 0 tables): position row 0 / token-type row 0 get no entry
int text_embed_bwd(hipStream_t st, int batch, int n_tok, int hidden, int vocab, int n_types, int n_tasks, const int64_t* ids,
                   const int64_t* seg, const int64_t* task_ids, const float* dx, float* dword, float* dpos, float* dtype,
                   float* dtask, bool skip_pos0, bool skip_type0);
}  // namespace vbemb

namespace vbrows {
// row kernels of an output + feed-forward block that runs on a subset of its rows (rowmap.hip; fp32, cols % 4 == 0):
// map[r] = the row of the full tensor compact row r stands for, -1 = padding row
int gather(hipStream_t st, long M, int cols, const float* src, const int32_t* map, long src_rows, float* out);
// out[r] = dropout(lin[r], p, mask of full row map[r]) + res[res_mapped ? map[r] : r] (out may be lin); res null: the
// dropped twin of a compact gradient, out[r] = keep(seed, map[r] cols + col) ? lin[r] / (1 - p) : 0, padding rows zeros
int drop_add(hipStream_t st, long M, int cols, const float* lin, const float* res, bool res_mapped, const int32_t* map,
             long src_rows, float* out, float p, uint64_t seed);
// inv[R] = the compact row with map[r] == R (the first, should there be more), or -1
int invert(hipStream_t st, long src_rows, long M, const int32_t* map, int32_t* inv);
// full[R] = compact[inv[R]] (compact: M rows), zeros where inv[R] is outside [0, M)
int scatter(hipStream_t st, long src_rows, int cols, const float* compact, long M, const int32_t* inv, float* full);
// the mover behind gather and scatter, of any element type: out[r] = src[map[r]] for r < rows in 16-byte chunks, zeros where
// map[r] is outside [0, src_rows); `chunks` per row, the row strides lds / ldo in 16-byte units, at most max_blocks blocks
int move_rows(hipStream_t st, long rows, int chunks, const void* src, long lds, long src_rows, const int32_t* map, void* out,
              long ldo, long max_blocks);
// out[j] += part[0][j] + part[1][j] + ... + part[parts - 1][j] in that order, j < n (bf16_helpers.hip)
int colsum_finish(hipStream_t st, long parts, int n, const float* part, long ldp, float* out);
}  // namespace vbrows

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// GELU (vilbert.py:117  x * 0.5 * (1 + erf(x / sqrt(2)))) and its derivative from ONE exponential:
//   z = |x| / sqrt 2,  E = exp(-z^2) = exp(-x^2 / 2),  erfc(z) = poly(t) t E with t = 1 / (1 + 0.3275911 z)
//   (Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 - three orders below the 1e-4 parity bar),
//   Phi(x) = x >= 0 ? 1 - erfc(z) / 2 : erfc(z) / 2 (no cancellation on the negative side),
//   gelu = x Phi,  gelu' = Phi + x E / sqrt(2 pi).
// ~20 VALU instructions for both values; libdevice's erff + expf cost ~55, which showed as 15 % of the FFN
// up-projection GEMM (28 M outputs per launch) and as 58 us of a 160 us fp8 GEMM.
__device__ __forceinline__ void gelu_parts(float x, float& phi, float& e) {
    const float z = fabsf(x) * 0.70710678118654752440f;
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
    e = __expf(-z * z);
    float poly = fmaf(1.061405429f, t, -1.453152027f);
    poly = fmaf(poly, t, 1.421413741f);
    poly = fmaf(poly, t, -0.284496736f);
    poly = fmaf(poly, t, 0.254829592f);
    const float half_erfc = 0.5f * poly * t * e;
    phi = x >= 0.f ? 1.0f - half_erfc : half_erfc;
}

__device__ __forceinline__ float gelu_erf(float x) {
    float phi, e;
    gelu_parts(x, phi, e);
    return x * phi;
}

__device__ __forceinline__ float gelu_grad(float x) {
    // d/dx [x Phi(x)] = Phi(x) + x exp(-x^2 / 2) / sqrt(2 pi)
    float phi, e;
    gelu_parts(x, phi, e);
    return fmaf(x * 0.39894228040143267794f, e, phi);
}

// both at once (the FFN up-projection epilogue in training stores the activation and its derivative)
__device__ __forceinline__ void gelu_and_grad(float x, float& y, float& d) {
    float phi, e;
    gelu_parts(x, phi, e);
    y = x * phi;
    d = fmaf(x * 0.39894228040143267794f, e, phi);
}

__device__ __forceinline__ float swish_act(float x) {
    // vilbert.py:120-121  x * sigmoid(x)
    return x / (1.0f + expf(-x));
}

__device__ __forceinline__ float swish_grad(float x) {
    const float s = 1.0f / (1.0f + expf(-x));
    return s + x * s * (1.0f - s);
}
