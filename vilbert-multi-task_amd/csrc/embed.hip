// Embedding row kernels: the fused text embedding gather + LayerNorm, the fused image location projection + LayerNorm, the
// additive-mask conversion, and the atomic (non-deterministic setting) scatter of the text embedding gradients - the ordered
// one is embed_bwd.hip. Row layout and the LayerNorm finish: rowops.h.
#include "rowops.h"

using namespace vbrow;

namespace {

// reference vilbert.py:346-367
template <int NV>
__global__ __launch_bounds__(256) void text_embed_kernel(int batch, int n_tok, int hidden, int vocab, int n_types,
                                                         int n_tasks, const int64_t* __restrict__ ids,
                                                         const int64_t* __restrict__ seg, int pos_offset,
                                                         const float* __restrict__ word,
                                                         const float* __restrict__ pos,
                                                         const float* __restrict__ type,
                                                         const int64_t* __restrict__ task_ids,
                                                         const float* __restrict__ task_emb,
                                                         const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps,
                                                         float* __restrict__ out, float* mean, float* rstd,
                                                         float* presum) {
    const int lane = threadIdx.x & 63;
    const int n_out = n_tok + (task_ids != nullptr ? 1 : 0);
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= (long)batch * n_out) return;
    const int b = (int)(row / n_out), t_out = (int)(row % n_out);
    // with task tokens: output 0 <- token 0, output 1 <- task embedding, output t <- token t - 1
    const bool is_task = task_ids != nullptr && t_out == 1;
    const int t = (task_ids != nullptr && t_out >= 2) ? t_out - 1 : t_out;
    // ids outside their table (the reference's nn.Embedding raises a device assert there) read nothing: the
    // row contributes zeros instead of whatever lies past the allocation
    const float *w = nullptr, *pp = nullptr, *ty = nullptr;
    if (is_task) {
        const int64_t k = task_ids[b];
        if (k >= 0 && k < n_tasks) w = task_emb + k * hidden;
    } else {
        const int64_t id = ids[(long)b * n_tok + t], sg = seg[(long)b * n_tok + t];
        if (id >= 0 && id < vocab) w = word + id * hidden;
        pp = pos + (long)(t + pos_offset) * hidden;
        if (sg >= 0 && sg < n_types) ty = type + sg * hidden;
    }
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (col < hidden) {
            if (w != nullptr) v[i] = *reinterpret_cast<const f32x4*>(w + col);
            if (!is_task) {
                // words + position + token_type, in the reference's order (vilbert.py:355)
                v[i] += *reinterpret_cast<const f32x4*>(pp + col);
                if (ty != nullptr) v[i] += *reinterpret_cast<const f32x4*>(ty + col);
            }
        }
    }
    ln_finish<NV>(v, hidden, lane, gamma, beta, eps, out + row * hidden, mean ? mean + row : nullptr,
                  rstd ? rstd + row : nullptr, presum ? presum + row * hidden : nullptr);
}

// reference vilbert.py:1421-1432 (the 5 -> hidden location projection, the sum and the LayerNorm)
template <int NV>
__global__ __launch_bounds__(256) void image_embed_kernel(long rows, int hidden,
                                                          const float* __restrict__ feat_proj,
                                                          const float* __restrict__ loc,
                                                          const float* __restrict__ w_loc,
                                                          const float* __restrict__ b_loc,
                                                          const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, float eps,
                                                          float* __restrict__ out, float* mean, float* rstd,
                                                          float* presum) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    float l[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) l[j] = loc[row * 5 + j];
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (col < hidden) {
            f32x4 lp = *reinterpret_cast<const f32x4*>(b_loc + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* wr = w_loc + (long)(col + e) * 5;
                float a = 0.f;
#pragma unroll
                for (int j = 0; j < 5; ++j) a = fmaf(l[j], wr[j], a);
                lp[e] += a;
            }
            v[i] = *reinterpret_cast<const f32x4*>(feat_proj + row * hidden + col) + lp;
        }
    }
    ln_finish<NV>(v, hidden, lane, gamma, beta, eps, out + row * hidden, mean ? mean + row : nullptr,
                  rstd ? rstd + row : nullptr, presum ? presum + row * hidden : nullptr);
}

template <typename T>
__global__ void additive_mask_kernel(long n, const T* __restrict__ mask, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    // reference vilbert.py:1353,1362: (1.0 - mask) * -10000.0
    if (i < n) out[i] = (1.0f - (float)mask[i]) * -10000.0f;
}

// Scatter-add of embedding-row gradients (fp32 atomics into the zero-filled tables).
// reference vilbert.py:353-362 backward; word row 0 is padding_idx (no gradient from the gather).
template <int NV>
__global__ __launch_bounds__(256) void text_embed_scatter_kernel(int batch, int n_tok, int hidden, int vocab,
                                                                 int n_tasks, const int64_t* __restrict__ ids,
                                                                 const int64_t* __restrict__ seg,
                                                                 const int64_t* __restrict__ task_ids,
                                                                 const float* __restrict__ dx,
                                                                 float* __restrict__ dword, float* __restrict__ dpos,
                                                                 float* __restrict__ dtype, float* __restrict__ dtask) {
    const int lane = threadIdx.x & 63;
    const int n_out = n_tok + (task_ids != nullptr ? 1 : 0);
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= (long)batch * n_out) return;
    const int b = (int)(row / n_out), t_out = (int)(row % n_out);
    const bool is_task = task_ids != nullptr && t_out == 1;
    const int t = (task_ids != nullptr && t_out >= 2) ? t_out - 1 : t_out;
    float* w = nullptr;
    if (is_task) {
        const int64_t k = task_ids[b];
        w = (k >= 0 && k < n_tasks) ? dtask + k * hidden : nullptr;
    } else {
        const int64_t id = ids[(long)b * n_tok + t];
        w = (id > 0 && id < vocab) ? dword + id * hidden : nullptr;
        // position / token-type rows are shared by every sample (36 + 2 rows for 9216 tokens): they are
        // reduced by pos_type_grad_kernel instead of 9216-way contended atomics
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        if (col < hidden) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(dx + row * hidden + col);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (w != nullptr) unsafeAtomicAdd(w + col + e, d[e]);
        }
    }
}

// dpos[t] += sum_b dx[b, t] and dtype[s] += sum over the tokens of type s: one block per token
// position walks the batch (coalesced rows), so dpos needs no atomics and dtype one per position.
__global__ __launch_bounds__(256) void pos_type_grad_kernel(int batch, int n_tok, int hidden, int n_types,
                                                            const int64_t* __restrict__ seg,
                                                            const int64_t* __restrict__ task_ids,
                                                            const float* __restrict__ dx,
                                                            float* __restrict__ dpos, float* __restrict__ dtype,
                                                            bool skip_pos0, bool skip_type0) {
    const int n_out = n_tok + (task_ids != nullptr ? 1 : 0);
    const int t_out = blockIdx.x;
    if (task_ids != nullptr && t_out == 1) return;  // the task-token row has no position / type
    const int t = (task_ids != nullptr && t_out >= 2) ? t_out - 1 : t_out;
    for (int col = threadIdx.x * 4; col < hidden; col += 256 * 4) {
        f32x4 ap = {0.f, 0.f, 0.f, 0.f}, a0 = ap, a1 = ap;
        for (int b = 0; b < batch; ++b) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(dx + ((long)b * n_out + t_out) * hidden + col);
            const int64_t ty = seg[(long)b * n_tok + t];
            ap += d;
            if (ty == 0) a0 += d;
            else if (ty == 1) a1 += d;
            else if (ty > 1 && ty < n_types) {
#pragma unroll
                for (int e = 0; e < 4; ++e) unsafeAtomicAdd(dtype + ty * hidden + col + e, d[e]);
            }
        }
        // the type table may hold a single row (roberta_base_6layer_6connect.json: type_vocab_size = 1)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // (skip_*: the baseline's padding_idx = 0 rows receive nothing - vbb_text_embed_bwd)
            if (!(skip_pos0 && t == 0)) unsafeAtomicAdd(dpos + (long)t * hidden + col + e, ap[e]);
            if (n_types > 0 && !skip_type0) unsafeAtomicAdd(dtype + col + e, a0[e]);
            if (n_types > 1) unsafeAtomicAdd(dtype + hidden + col + e, a1[e]);
        }
    }
}

}  // namespace

extern "C" int vb_text_embed_ln_fwd(void* stream, int32_t batch, int32_t n_tok, int32_t hidden, int32_t vocab,
                                    int32_t n_types, int32_t n_tasks,
                                    const int64_t* ids, const int64_t* seg, int32_t pos_offset,
                                    const float* word_emb, const float* pos_emb, const float* type_emb,
                                    const int64_t* task_ids, const float* task_emb, const float* gamma,
                                    const float* beta, float eps, float* out, float* mean, float* rstd,
                                    float* presum) {
    if (any_null({ids, seg, word_emb, pos_emb, type_emb, gamma, beta, out}) || batch <= 0 || n_tok <= 0 || vocab <= 0 ||
        n_types <= 0)
        return VB_E_BADARG;
    if (task_ids != nullptr && (task_emb == nullptr || n_tasks <= 0)) return VB_E_BADARG;
    if (int e = check_cols(hidden)) return e;
    if (!all_aligned(16, {word_emb, pos_emb, type_emb, out, gamma, beta, task_emb})) return VB_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long rows = (long)batch * (n_tok + (task_ids != nullptr ? 1 : 0));
    dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(256);
    dispatch_nv<32>(nv_for(hidden), [&](auto nv) {
        hipLaunchKernelGGL((text_embed_kernel<decltype(nv)::value>), grid, block, 0, st, batch, n_tok, hidden, vocab, n_types,
                           n_tasks, ids, seg, pos_offset, word_emb, pos_emb, type_emb, task_ids, task_emb, gamma, beta, eps,
                           out, mean, rstd, presum);
    });
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_image_embed_ln_fwd(void* stream, int64_t rows, int32_t hidden, const float* feat_proj,
                                     const float* loc, const float* w_loc, const float* b_loc,
                                     const float* gamma, const float* beta, float eps, float* out, float* mean,
                                     float* rstd, float* presum) {
    if (any_null({feat_proj, loc, w_loc, b_loc, gamma, beta, out}) || rows <= 0) return VB_E_BADARG;
    if (int e = check_cols(hidden)) return e;
    if (!all_aligned(16, {feat_proj, out, b_loc, gamma, beta})) return VB_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(256);
    dispatch_nv<32>(nv_for(hidden), [&](auto nv) {
        hipLaunchKernelGGL((image_embed_kernel<decltype(nv)::value>), grid, block, 0, st, (long)rows, hidden, feat_proj, loc,
                           w_loc, b_loc, gamma, beta, eps, out, mean, rstd, presum);
    });
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_additive_mask(void* stream, int64_t n, const void* mask, int32_t mask_is_f32, float* out) {
    if (mask == nullptr || out == nullptr || n <= 0) return VB_E_BADARG;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (mask_is_f32)
        hipLaunchKernelGGL(additive_mask_kernel<float>, grid, block, 0, st, (long)n,
                           static_cast<const float*>(mask), out);
    else
        hipLaunchKernelGGL(additive_mask_kernel<int64_t>, grid, block, 0, st, (long)n,
                           static_cast<const int64_t*>(mask), out);
    VB_LAUNCH_CHECK();
    return 0;
}

int vbemb::text_embed_bwd(hipStream_t st, int batch, int n_tok, int hidden, int vocab, int n_types, int n_tasks,
                          const int64_t* ids, const int64_t* seg, const int64_t* task_ids, const float* dx, float* dword,
                          float* dpos, float* dtype, float* dtask, bool skip_pos0, bool skip_type0) {
    if (any_null({ids, seg, dx, dword, dpos, dtype}) || batch <= 0 || n_tok <= 0 || vocab <= 0 || n_types <= 0)
        return VB_E_BADARG;
    if (task_ids != nullptr && (dtask == nullptr || n_tasks <= 0)) return VB_E_BADARG;
    if (int e = check_cols(hidden)) return e;
    if (!vb_aligned16(dx)) return VB_E_ALIGN;
    // deterministic setting: the ordered keyed reduction (embed_bwd.hip); without a workspace slice, the atomics below
    const int ordered = vbemb::text_embed_bwd_det(st, batch, n_tok, hidden, vocab, n_types, n_tasks, ids, seg, task_ids,
                                                  dx, dword, dpos, dtype, dtask, skip_pos0, skip_type0);
    if (ordered >= 0) return ordered;
    const long rows = (long)batch * (n_tok + (task_ids != nullptr ? 1 : 0));
    dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(256);
    dispatch_nv<32>(nv_for(hidden), [&](auto nv) {
        hipLaunchKernelGGL((text_embed_scatter_kernel<decltype(nv)::value>), grid, block, 0, st, batch, n_tok, hidden, vocab,
                           n_tasks, ids, seg, task_ids, dx, dword, dpos, dtype, dtask);
    });
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(pos_type_grad_kernel, dim3((unsigned)(n_tok + (task_ids != nullptr ? 1 : 0))), dim3(256), 0,
                       st, batch, n_tok, hidden, n_types, seg, task_ids, dx, dpos, dtype, skip_pos0, skip_type0);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_text_embed_bwd(void* stream, int32_t batch, int32_t n_tok, int32_t hidden, int32_t vocab,
                                 int32_t n_types, int32_t n_tasks, const int64_t* ids, const int64_t* seg,
                                 const int64_t* task_ids, const float* dx, float* dword, float* dpos, float* dtype,
                                 float* dtask) {
    return vbemb::text_embed_bwd(static_cast<hipStream_t>(stream), batch, n_tok, hidden, vocab, n_types, n_tasks, ids, seg,
                                 task_ids, dx, dword, dpos, dtype, dtask, false, false);
}
