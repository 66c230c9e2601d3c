// fp32 -> bf16, round to nearest even: the ONE place every bf16 store of the library takes its rounding from (the GEMM
// epilogues of gemm_bf16.hip, the cast / shadow kernels of bf16_helpers.hip, layernorm.hip, mx8.hip, attention.hip
// in its bf16 build, attention_mx.hip). No HIP header and no device state. One name, two bodies with one contract:
//   * device code for gfx950 - every kernel of the library - is the hardware convert v_cvt_pk_bf16_f32;
//   * host code, and device code for any other architecture, is the integer add-and-shift the kernels used to carry in
//     eight copies, with a NaN case in front of it.
// Contract: a finite value or +-Inf rounds to nearest even exactly as torch's CPU cast does (subnormal inputs and results
// included: nothing is flushed; the largest finites carry into Inf); a NaN stays a NaN (quiet, sign kept). The add-and-shift
// alone turned 0x7f800001 .. 0x7f80ffff into +Inf and wrapped 0x7fff8000 .. 0x7fffffff / 0xffff8000 .. 0xffffffff to -0 / +0 -
// an overflowed step then looked finite to the optimizer's skip_nonfinite check.
// Who checks what: tests/test_bf16_round.py compiles this header with the host compiler and holds the INTEGER body to the
// contract over every rounding decision (65,536 upper halves x 8 lower halves) - a path no kernel executes;
// tests/test_bf16_helpers_gpu.py holds the DEVICE body to the same contract over the same patterns through the cast and
// shadow kernels. That the two bodies agree bit for bit on every non-NaN input follows from both tests, not from either.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define VB_BF16_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define VB_BF16_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
// device: the hardware convert (v_cvt_pk_bf16_f32, two values per instruction) - round to nearest even, subnormals kept
// (the kernels run with fp32 denormals on), NaN -> quiet NaN. The integer form with its select was measured first: 4 % under
// the parent commit on the bf16 training step and 7 % on the MX forward, this form level with or above the parent
// (profiles/bf16_round_ab.txt) - the GEMM epilogues are not store-bound.
typedef float vb_f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 vb_bf16x2_t __attribute__((ext_vector_type(2)));

// two values in one 32-bit word: lo in bits 0 .. 15, hi in bits 16 .. 31 (adjacent columns of a row)
VB_BF16_FN uint32_t vb_bf16_pack(float lo, float hi) {
    return __builtin_bit_cast(uint32_t, __builtin_convertvector((vb_f32x2_t){lo, hi}, vb_bf16x2_t));
}

VB_BF16_FN uint32_t vb_bf16_round(float v) { return vb_bf16_pack(v, v) & 0xffffu; }
#else
// host, other architectures: the same rounding in integer arithmetic. The word's UPPER half is the bf16 value (the lower half is rubbish): the
// select sits in front of the shift, so that a pair packs with one mask-and-merge
VB_BF16_FN uint32_t vb_bf16_round_word(float v) {
    const uint32_t u = __builtin_bit_cast(uint32_t, v);
    return v != v ? u | 0x00400000u : u + 0x7fffu + ((u >> 16) & 1u);
}

VB_BF16_FN uint32_t vb_bf16_round(float v) { return vb_bf16_round_word(v) >> 16; }

VB_BF16_FN uint32_t vb_bf16_pack(float lo, float hi) {
    return (vb_bf16_round_word(lo) >> 16) | (vb_bf16_round_word(hi) & 0xffff0000u);
}
#endif

#undef VB_BF16_FN
