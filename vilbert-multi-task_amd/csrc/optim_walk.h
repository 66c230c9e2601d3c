// The chunk walk of the multi-tensor optimizer kernels (optimizer.hip, lamb.hip). One block of 256 threads per chunk: chunk c
// covers elements [chunk_off[c], chunk_off[c] + chunk_elems) of tensor chunk_tensor[c] of the vb_adamw_tensor table. A kernel
// is: grad_state (coefficient / skipped step), chunk_of_block, walk<LOADS, STORES, RULE> with its element function, and for
// the two kernels that reduce, block_sum.
//
// A tensor's bits depend on two rules stated here and nowhere else:
//  - 16-byte or scalar access is chosen for a whole chunk from the tensor's BASE pointers (chunk offsets are multiples of 4
//    elements). The update kernels and both LAMB stages test all four pointers (ALIGN_ALL) - also one the kernel does not
//    touch, so that both LAMB stages walk a chunk the same way. The one exception is the norm pass, which tests the gradient
//    alone (ALIGN_GRAD): a tensor whose parameter is an oddly offset view still has its gradient summed with 16-byte loads.
//  - element e of the vector path belongs to lane e % 4, every element of the scalar path to lane 0: a reducing kernel keeps
//    one accumulator per lane (four chains on the vector path, one on the scalar path), combines them with lane_sum and the
//    block's values with block_sum.
#pragma once
#include <initializer_list>

#include "common.h"
#include "../../include/vilbert_hip_ext.h"  // the state of the norm pass

namespace optim_walk {

enum : unsigned { P = 1, G = 2, M = 4, V = 8, ALIGN_ALL = P | G | M | V, ALIGN_GRAD = G };

// Argument check the entry points share: the launch tables and the chunk size, plus the entry point's own required pointers.
inline int check_tables(int32_t n_chunks, const vb_adamw_tensor* table, const int32_t* chunk_tensor, const int64_t* chunk_off,
                        int32_t chunk_elems, std::initializer_list<const void*> required = {}) {
    if (table == nullptr || chunk_tensor == nullptr || chunk_off == nullptr || n_chunks <= 0) return VB_E_BADARG;
    for (const void* ptr : required)
        if (ptr == nullptr) return VB_E_BADARG;
    if (chunk_elems <= 0 || chunk_elems % 4 != 0) return VB_E_ALIGN;
    return 0;
}

struct Chunk {
    int ti;               // row of the tensor table(s)
    vb_adamw_tensor t;
    long off, end;        // the block's elements of t
};

__device__ __forceinline__ Chunk chunk_of_block(const vb_adamw_tensor* __restrict__ tab, const int32_t* __restrict__ chunk_tensor,
                                                const int64_t* __restrict__ chunk_off, int chunk_elems) {
    Chunk c;
    c.ti = chunk_tensor[blockIdx.x];
    c.t = tab[c.ti];
    c.off = chunk_off[blockIdx.x];
    c.end = min((long)c.t.numel, c.off + chunk_elems);
    return c;
}

// The coefficient every gradient is multiplied by as it is loaded; false = the block belongs to a skipped step and returns
// before any store. `state` (written by grad_norm_finish_kernel) == nullptr is the plain step: coefficient 1 - it multiplies
// exactly - and never skipped. Read once per block, uniform branches.
__device__ __forceinline__ bool grad_state(const float* __restrict__ state, int skip, float& coef) {
    coef = 1.0f;
    if (state == nullptr) return true;
    if (skip && state[VB_GRAD_STATE_FINITE] == 0.f) return false;
    coef = state[VB_GRAD_STATE_COEF];
    return true;
}

// Whether a chunk of `t` is walked with 16-byte accesses: the base pointers RULE names (ALIGN_ALL or ALIGN_GRAD) are aligned.
template <unsigned RULE>
__device__ __forceinline__ bool aligned16(const vb_adamw_tensor& t) {
    const uintptr_t bases = (RULE & P ? reinterpret_cast<uintptr_t>(t.param) : 0) | (RULE & G ? reinterpret_cast<uintptr_t>(t.grad) : 0) |
                            (RULE & M ? reinterpret_cast<uintptr_t>(t.exp_avg) : 0) | (RULE & V ? reinterpret_cast<uintptr_t>(t.exp_avg_sq) : 0);
    return (bases & 15u) == 0;
}

// f(lane, p, g, m, v) for every element of the chunk: the f32x4 loop with stride 256, then the scalar tail. Only the arrays
// in LOADS are read (the others arrive as 0), only those in STORES written; g arrives multiplied by coef. UNROLL is the
// unroll count of the vector loop. `reduce` gets the same arguments after the lane's results are in the vectors to store: a
// kernel that also sums accumulates there. The place matters - the compiler pairs the lanes of a round into packed
// instructions and fuses a * b + c per lane as the pairing allows, and with the accumulation in front of the write-back it
// fuses other multiply-adds of the element function (LAMB stage 1: other bits).
template <unsigned LOADS, unsigned STORES, unsigned RULE, int UNROLL = 1, class F, class R>
__device__ __forceinline__ void walk(const Chunk& c, float coef, F&& f, R&& reduce) {
    static_assert((STORES & (G | ~LOADS)) == 0, "the gradients are only read; a stored array is loaded first");
    float* __restrict__ p = c.t.param;
    const float* __restrict__ g = c.t.grad;
    float* __restrict__ m = c.t.exp_avg;
    float* __restrict__ v = c.t.exp_avg_sq;
    const long n4 = aligned16<RULE>(c.t) ? (c.end - c.off) >> 2 : 0;
#pragma unroll UNROLL
    for (long i = threadIdx.x; i < n4; i += 256) {
        const long e = c.off + 4 * i;
        f32x4 pp = {0.f, 0.f, 0.f, 0.f}, gg = pp, mm = pp, vv = pp;
        if constexpr (LOADS & P) pp = *reinterpret_cast<const f32x4*>(p + e);
        if constexpr (LOADS & G) gg = *reinterpret_cast<const f32x4*>(g + e) * coef;
        if constexpr (LOADS & M) mm = *reinterpret_cast<const f32x4*>(m + e);
        if constexpr (LOADS & V) vv = *reinterpret_cast<const f32x4*>(v + e);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float pk = pp[k], mk = mm[k], vk = vv[k];
            f(k, pk, gg[k], mk, vk);
            pp[k] = pk; mm[k] = mk; vv[k] = vk;
            reduce(k, pk, gg[k], mk, vk);
        }
        if constexpr (STORES & P) *reinterpret_cast<f32x4*>(p + e) = pp;
        if constexpr (STORES & M) *reinterpret_cast<f32x4*>(m + e) = mm;
        if constexpr (STORES & V) *reinterpret_cast<f32x4*>(v + e) = vv;
    }
    for (long e = c.off + 4 * n4 + threadIdx.x; e < c.end; e += 256) {
        float pp = 0.f, gg = 0.f, mm = 0.f, vv = 0.f;
        if constexpr (LOADS & P) pp = p[e];
        if constexpr (LOADS & G) gg = g[e] * coef;
        if constexpr (LOADS & M) mm = m[e];
        if constexpr (LOADS & V) vv = v[e];
        f(0, pp, gg, mm, vv);
        reduce(0, pp, gg, mm, vv);
        if constexpr (STORES & P) p[e] = pp;
        if constexpr (STORES & M) m[e] = mm;
        if constexpr (STORES & V) v[e] = vv;
    }
}

template <unsigned LOADS, unsigned STORES, unsigned RULE, int UNROLL = 1, class F>
__device__ __forceinline__ void walk(const Chunk& c, float coef, F&& f) {
    walk<LOADS, STORES, RULE, UNROLL>(c, coef, f, [](int, float, float, float, float) {});
}

// the per-lane accumulators of one thread, lanes 0..3
__device__ __forceinline__ float lane_sum(f32x4 acc) { return (acc[0] + acc[1]) + (acc[2] + acc[3]); }

// Block-wide sums of N values in a fixed order: the xor tree of each wave, then waves 0..3 through LDS as (w0 + w1) + (w2 + w3);
// thread 0 stores out[0 .. N).
template <int N>
__device__ __forceinline__ void block_sum(const float (&val)[N], float* __restrict__ out) {
    __shared__ float wave_part[N][4];
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float s = wave_sum(val[k]);
        if ((threadIdx.x & 63) == 0) wave_part[k][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) out[k] = (wave_part[k][0] + wave_part[k][1]) + (wave_part[k][2] + wave_part[k][3]);
    }
}

}  // namespace optim_walk
