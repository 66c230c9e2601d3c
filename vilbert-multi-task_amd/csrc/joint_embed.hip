// Kernels of the single-stream baseline (vilbert/basebert.py; C ABI in include/vilbert_hip_baseline.h, prefix vbb_): the joint
// text + image embedding that writes both segments of a sample into one [B, T + R, H] buffer, the backward of its two
// LayerNorms with per-segment column sums, the table scatter with the baseline's padding rows (the kernels are embed.hip's and
// embed_bwd.hip's) and the tanh of the pooler. Row layout and the LayerNorm finish: rowops.h.
#include "../../include/vilbert_hip_baseline.h"
#include "rowops.h"

using namespace vbrow;

namespace {

// (1 - m) * -10000 of one mask element; a null mask is all ones
__device__ __forceinline__ float additive(const void* mask, int is_f32, long i) {
    if (mask == nullptr) return (1.0f - 1.0f) * -10000.0f;
    const float m = is_f32 ? static_cast<const float*>(mask)[i] : (float)static_cast<const int64_t*>(mask)[i];
    return (1.0f - m) * -10000.0f;
}

struct JointText {
    const int64_t* ids;
    const int64_t* seg;
    const float* word;
    const float* pos;
    const float* type;
    const float* gamma;
    const float* beta;
    const void* mask;
    int vocab, n_types, mask_is_f32;
};

struct JointImage {
    const float* feat_proj;
    const float* loc;
    const float* w_loc;
    const float* b_loc;
    const float* type_row;
    const float* gamma;
    const float* beta;
    const void* mask;
    int mask_is_f32;
};

// reference basebert.py:305-321 (text), :342-359 (image), :735-762 (the two additive masks, concatenated)
template <int NV>
__global__ __launch_bounds__(256) void joint_embed_kernel(int batch, int n_tok, int n_reg, int hidden, JointText tx,
                                                          JointImage im, float eps, float* __restrict__ out, float* mean,
                                                          float* rstd, float* presum, float* __restrict__ add_mask) {
    const int lane = threadIdx.x & 63;
    const int n_out = n_tok + n_reg;
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= (long)batch * n_out) return;
    const int b = (int)(row / n_out), j = (int)(row % n_out);
    const bool text = j < n_tok;   // (wave-uniform)
    f32x4 v[NV];
    if (text) {
        const long tok = (long)b * n_tok + j;
        const int64_t id = tx.ids[tok], sg = tx.seg[tok];
        // ids outside their table read nothing: the row contributes zeros (as vb_text_embed_ln_fwd)
        const float* w = (id >= 0 && id < tx.vocab) ? tx.word + id * hidden : nullptr;
        const float* pp = tx.pos + (long)j * hidden;
        const float* ty = (sg >= 0 && sg < tx.n_types) ? tx.type + sg * hidden : nullptr;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (col < hidden) {
                if (w != nullptr) v[i] = *reinterpret_cast<const f32x4*>(w + col);
                v[i] += *reinterpret_cast<const f32x4*>(pp + col);
                if (ty != nullptr) v[i] += *reinterpret_cast<const f32x4*>(ty + col);
            }
        }
        if (lane == 0) add_mask[row] = additive(tx.mask, tx.mask_is_f32, tok);
    } else {
        const long reg = (long)b * n_reg + (j - n_tok);
        float l[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) l[q] = im.loc[reg * 5 + q];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (col < hidden) {
                f32x4 lp = *reinterpret_cast<const f32x4*>(im.b_loc + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float* wr = im.w_loc + (long)(col + e) * 5;
                    float a = 0.f;
#pragma unroll
                    for (int q = 0; q < 5; ++q) a = fmaf(l[q], wr[q], a);
                    lp[e] += a;
                }
                // image + token_type + location, in the reference's order (basebert.py:355)
                v[i] = (*reinterpret_cast<const f32x4*>(im.feat_proj + reg * hidden + col) +
                        *reinterpret_cast<const f32x4*>(im.type_row + col)) + lp;
            }
        }
        if (lane == 0) add_mask[row] = additive(im.mask, im.mask_is_f32, reg);
    }
    ln_finish<NV>(v, hidden, lane, text ? tx.gamma : im.gamma, text ? tx.beta : im.beta, eps, out + row * hidden,
                  mean ? mean + row : nullptr, rstd ? rstd + row : nullptr, presum ? presum + row * hidden : nullptr);
}

// ------------------------------------------------------------------------------------------------
// Backward (the arithmetic of layernorm_bwd_kernel): per row, xhat = (x - mean) rstd, g = dy * gamma,
//   dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  dgamma = sum_rows dy * xhat,  dbeta = sum_rows dy
// with the column sums taken PER SEGMENT. Rows are enumerated segment by segment: segment row s of the text segment is
// the joint row (s / n_tok) (n_tok + n_reg) + s % n_tok and lands in dx_text[s], likewise the image segment behind
// n_tok. A block (4 waves x JB_ROWS_PER_WAVE rows) covers consecutive rows of ONE segment, so its partial belongs to one
// pair of column sums: blocks [0, nb_t) are text, [nb_t, nb_t + nb_v) image.
// ------------------------------------------------------------------------------------------------
constexpr int JB_ROWS_PER_WAVE = 4;
constexpr int JB_ROWS_PER_BLOCK = 4 * JB_ROWS_PER_WAVE;
constexpr int JB_MAX_REG_COLS = 1024;   // wider rows: one workspace partial per row (joint_embed_bwd_wide_kernel)

inline long jb_blocks(long seg_rows) { return (seg_rows + JB_ROWS_PER_BLOCK - 1) / JB_ROWS_PER_BLOCK; }

struct JointSeg {
    long seg_rows;      // batch * n_seg
    int n_seg, offset;  // rows of the segment per sample, first joint row of the segment inside a sample
    const float* gamma;
    float* dx;
};

__device__ __forceinline__ long joint_row(const JointSeg& sg, long s, int n_out) {
    return (s / sg.n_seg) * n_out + sg.offset + s % sg.n_seg;
}

template <int NV>
__global__ __launch_bounds__(256) void joint_embed_bwd_kernel(long nb_t, int n_out, int n_cols, JointSeg st, JointSeg sv,
                                                              const float* __restrict__ dy, const float* __restrict__ x,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd, float* __restrict__ ws) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool text = (long)blockIdx.x < nb_t;   // (block-uniform)
    const JointSeg& sg = text ? st : sv;
    const long row_begin = ((long)blockIdx.x - (text ? 0 : nb_t)) * JB_ROWS_PER_BLOCK + wave * JB_ROWS_PER_WAVE;
    f32x4 gam[NV], dg[NV], db[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        gam[i] = col < n_cols ? *reinterpret_cast<const f32x4*>(sg.gamma + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        dg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int rr = 0; rr < JB_ROWS_PER_WAVE; ++rr) {
        const long s = row_begin + rr;
        if (s >= sg.seg_rows) break;
        const long row = joint_row(sg, s, n_out);
        const float mu = mean[row], rs = rstd[row];
        f32x4 xh[NV], g[NV];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            xh[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            g[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (col < n_cols) {
                const f32x4 d = *reinterpret_cast<const f32x4*>(dy + row * n_cols + col);
                xh[i] = (*reinterpret_cast<const f32x4*>(x + row * n_cols + col) - mu) * rs;
                g[i] = d * gam[i];
                dg[i] += d * xh[i];
                db[i] += d;
                s1 += (g[i][0] + g[i][1]) + (g[i][2] + g[i][3]);
                s2 += (g[i][0] * xh[i][0] + g[i][1] * xh[i][1]) + (g[i][2] * xh[i][2] + g[i][3] * xh[i][3]);
            }
        }
        const float m1 = wave_sum(s1) / (float)n_cols, m2 = wave_sum(s2) / (float)n_cols;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            if (col < n_cols) *reinterpret_cast<f32x4*>(sg.dx + s * n_cols + col) = (g[i] - m1 - xh[i] * m2) * rs;
        }
    }
    // the four waves of the block, added in wave order: one workspace row [dgamma | dbeta] per block
    __shared__ f32x4 red[3 * 2 * NV * 64];
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            red[((wave - 1) * 2 * NV + i) * 64 + lane] = dg[i];
            red[((wave - 1) * 2 * NV + NV + i) * 64 + lane] = db[i];
        }
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int w2 = 0; w2 < 3; ++w2)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            dg[i] += red[(w2 * 2 * NV + i) * 64 + lane];
            db[i] += red[(w2 * 2 * NV + NV + i) * 64 + lane];
        }
    float* w = ws + (long)blockIdx.x * 2 * n_cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        if (col < n_cols) {
            *reinterpret_cast<f32x4*>(w + col) = dg[i];
            *reinterpret_cast<f32x4*>(w + n_cols + col) = db[i];
        }
    }
}

// Rows wider than JB_MAX_REG_COLS (no baseline config; the C ABI takes up to VB_MAX_LN_COLS): one wave per segment row, the
// row walked twice in 256-column chunks, its dgamma / dbeta terms written straight to the workspace - one partial per row,
// text rows first (workspace row s), image rows behind them (st.seg_rows + s).
__global__ __launch_bounds__(256) void joint_embed_bwd_wide_kernel(int n_out, int n_cols, JointSeg st, JointSeg sv,
                                                                   const float* __restrict__ dy,
                                                                   const float* __restrict__ x,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd,
                                                                   float* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const long p = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= st.seg_rows + sv.seg_rows) return;
    const bool text = p < st.seg_rows;
    const JointSeg& sg = text ? st : sv;
    const long s = text ? p : p - st.seg_rows;
    const long row = joint_row(sg, s, n_out);
    const float mu = mean[row], rs = rstd[row];
    const float* __restrict__ dyr = dy + row * n_cols;
    const float* __restrict__ xr = x + row * n_cols;
    float s1 = 0.f, s2 = 0.f;
    for (int col = lane * 4; col < n_cols; col += 256) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(dyr + col);
        const f32x4 xh = (*reinterpret_cast<const f32x4*>(xr + col) - mu) * rs;
        const f32x4 g = d * *reinterpret_cast<const f32x4*>(sg.gamma + col);
        s1 += (g[0] + g[1]) + (g[2] + g[3]);
        s2 += (g[0] * xh[0] + g[1] * xh[1]) + (g[2] * xh[2] + g[3] * xh[3]);
    }
    const float m1 = wave_sum(s1) / (float)n_cols, m2 = wave_sum(s2) / (float)n_cols;
    float* __restrict__ w = ws + p * 2 * n_cols;
    for (int col = lane * 4; col < n_cols; col += 256) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(dyr + col);
        const f32x4 xh = (*reinterpret_cast<const f32x4*>(xr + col) - mu) * rs;
        const f32x4 g = d * *reinterpret_cast<const f32x4*>(sg.gamma + col);
        *reinterpret_cast<f32x4*>(sg.dx + s * n_cols + col) = (g - m1 - xh * m2) * rs;
        *reinterpret_cast<f32x4*>(w + col) = d * xh;
        *reinterpret_cast<f32x4*>(w + n_cols + col) = d;
    }
}

// Stage 2: blockIdx.y = segment (0 text: workspace rows [0, parts_t), 1 image: the parts_v rows behind them); column sums of
// the segment's partial rows of width 2 n_cols -> [dgamma | dbeta]. 16 row groups x 64 columns: group g adds the parts g,
// g + 16, ... in that order, then the 16 groups are added in order through LDS.
__global__ __launch_bounds__(1024) void joint_colreduce_kernel(long parts_t, long parts_v, int n_cols,
                                                               const float* __restrict__ ws, float* __restrict__ dg_t,
                                                               float* __restrict__ db_t, float* __restrict__ dg_v,
                                                               float* __restrict__ db_v) {
    __shared__ float red[16][64];
    const int c = threadIdx.x & 63, pg = threadIdx.x >> 6;
    const int width = 2 * n_cols;
    const int col = blockIdx.x * 64 + c;
    const bool text = blockIdx.y == 0;
    const long parts = text ? parts_t : parts_v;
    const float* __restrict__ base = ws + (text ? 0 : parts_t) * width;
    float s0 = 0.f;
    if (col < width)
        for (long p = pg; p < parts; p += 16) s0 += base[p * width + col];
    red[pg][c] = s0;
    __syncthreads();
    if (pg == 0 && col < width) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i][c];
        if (col < n_cols) (text ? dg_t : dg_v)[col] = t;
        else (text ? db_t : db_v)[col - n_cols] = t;
    }
}

__global__ __launch_bounds__(256) void tanh_fwd_kernel(long n, const float* x, float* y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) y[i] = tanhf(x[i]);
}

__global__ __launch_bounds__(256) void tanh_bwd_kernel(long n, const float* dy, const float* y, float* dx) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float t = y[i];
        dx[i] = dy[i] * (1.0f - t * t);
    }
}

// sizes shared by the forward, the backward and the workspace query: 0 = ok and *rows = batch * (n_tok + n_reg)
int joint_sizes(int batch, int n_tok, int n_reg, int hidden, long* rows) {
    if (batch < 0 || n_tok <= 0 || n_reg <= 0) return VB_E_BADARG;
    if (int e = check_cols(hidden)) return e;
    long r = 0, elems = 0;
    if (__builtin_mul_overflow((long)batch, (long)n_tok + (long)n_reg, &r) || __builtin_mul_overflow(r, (long)hidden, &elems) ||
        __builtin_mul_overflow(elems, 8L, &elems))   // (bytes of a [rows, 2 hidden] fp32 workspace still fit)
        return VB_E_RANGE;
    if (r > 4L * 0x7fffffffL) return VB_E_RANGE;   // (one wave per row, 4 rows per block)
    *rows = r;
    return 0;
}

// partial rows of a segment in the workspace
inline long jb_parts(long seg_rows, int hidden) { return hidden > JB_MAX_REG_COLS ? seg_rows : jb_blocks(seg_rows); }

}  // namespace

extern "C" int vbb_joint_embed_fwd(void* stream, int32_t batch, int32_t n_tok, int32_t n_reg, int32_t hidden, int32_t vocab,
                                   int32_t n_types, const int64_t* ids, const int64_t* seg, const float* word_emb,
                                   const float* pos_emb, const float* type_emb, const float* gamma_t, const float* beta_t,
                                   const float* feat_proj, const float* loc, const float* w_loc, const float* b_loc,
                                   const float* type_row, const float* gamma_v, const float* beta_v, float eps,
                                   const void* mask_t, int32_t mask_t_is_f32, const void* mask_v, int32_t mask_v_is_f32,
                                   float* out, float* mean, float* rstd, float* presum, float* add_mask) {
    if (any_null({ids, seg, word_emb, pos_emb, type_emb, gamma_t, beta_t, feat_proj, loc, w_loc, b_loc, type_row, gamma_v,
                  beta_v, out, add_mask}) ||
        vocab <= 0 || n_types <= 0)
        return VB_E_BADARG;
    long rows = 0;
    if (int e = joint_sizes(batch, n_tok, n_reg, hidden, &rows)) return e;
    if (!all_aligned(16, {word_emb, pos_emb, type_emb, gamma_t, beta_t, feat_proj, b_loc, type_row, gamma_v, beta_v, out,
                          presum}))
        return VB_E_ALIGN;
    if (rows == 0) return 0;
    const JointText tx{ids, seg, word_emb, pos_emb, type_emb, gamma_t, beta_t, mask_t, vocab, n_types, mask_t_is_f32};
    const JointImage im{feat_proj, loc, w_loc, b_loc, type_row, gamma_v, beta_v, mask_v, mask_v_is_f32};
    hipStream_t st = static_cast<hipStream_t>(stream);
    dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(256);
    dispatch_nv<32>(nv_for(hidden), [&](auto nv) {
        hipLaunchKernelGGL((joint_embed_kernel<decltype(nv)::value>), grid, block, 0, st, batch, n_tok, n_reg, hidden, tx, im,
                           eps, out, mean, rstd, presum, add_mask);
    });
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vbb_joint_embed_bwd_workspace(int32_t batch, int32_t n_tok, int32_t n_reg, int32_t hidden) {
    long rows = 0;
    if (joint_sizes(batch, n_tok, n_reg, hidden, &rows) != 0) return 0;
    return (jb_parts((long)batch * n_tok, hidden) + jb_parts((long)batch * n_reg, hidden)) * 2 * hidden;
}

extern "C" int vbb_joint_embed_bwd(void* stream, int32_t batch, int32_t n_tok, int32_t n_reg, int32_t hidden,
                                   const float* dy, const float* presum, const float* mean, const float* rstd,
                                   const float* gamma_t, const float* gamma_v, float* dx_text, float* dx_img,
                                   float* dgamma_t, float* dbeta_t, float* dgamma_v, float* dbeta_v, float* workspace) {
    if (any_null({dy, presum, mean, rstd, gamma_t, gamma_v, dx_text, dx_img, dgamma_t, dbeta_t, dgamma_v, dbeta_v, workspace}))
        return VB_E_BADARG;
    long rows = 0;
    if (int e = joint_sizes(batch, n_tok, n_reg, hidden, &rows)) return e;
    if (!all_aligned(16, {dy, presum, gamma_t, gamma_v, dx_text, dx_img, workspace})) return VB_E_ALIGN;
    if (rows == 0) return 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_out = n_tok + n_reg;
    const JointSeg sgt{(long)batch * n_tok, n_tok, 0, gamma_t, dx_text};
    const JointSeg sgv{(long)batch * n_reg, n_reg, n_tok, gamma_v, dx_img};
    const long parts_t = jb_parts(sgt.seg_rows, hidden), parts_v = jb_parts(sgv.seg_rows, hidden);
    if (hidden > JB_MAX_REG_COLS) {
        hipLaunchKernelGGL(joint_embed_bwd_wide_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, n_out, hidden, sgt,
                           sgv, dy, presum, mean, rstd, workspace);
    } else {
        const dim3 grid((unsigned)(parts_t + parts_v)), block(256);
        dispatch_nv<4>(nv_for(hidden), [&](auto nv) {
            hipLaunchKernelGGL((joint_embed_bwd_kernel<decltype(nv)::value>), grid, block, 0, st, parts_t, n_out, hidden, sgt,
                               sgv, dy, presum, mean, rstd, workspace);
        });
    }
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(joint_colreduce_kernel, dim3((unsigned)((2 * hidden + 63) / 64), 2), dim3(1024), 0, st, parts_t, parts_v,
                       hidden, (const float*)workspace, dgamma_t, dbeta_t, dgamma_v, dbeta_v);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbb_text_embed_bwd(void* stream, int32_t batch, int32_t n_tok, int32_t hidden, int32_t vocab, int32_t n_types,
                                  int32_t n_tasks, const int64_t* ids, const int64_t* seg, const int64_t* task_ids,
                                  const float* dx, float* dword, float* dpos, float* dtype, float* dtask, int32_t skip_pos0,
                                  int32_t skip_type0) {
    return vbemb::text_embed_bwd(static_cast<hipStream_t>(stream), batch, n_tok, hidden, vocab, n_types, n_tasks, ids, seg,
                                 task_ids, dx, dword, dpos, dtype, dtask, skip_pos0 != 0, skip_type0 != 0);
}

extern "C" int vbb_tanh_fwd(void* stream, int64_t n, const float* x, float* y) {
    if (x == nullptr || y == nullptr || n < 0) return VB_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(tanh_fwd_kernel, dim3(vb_grid_for(n, 256, 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), (long)n,
                       x, y);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vbb_tanh_bwd(void* stream, int64_t n, const float* dy, const float* y, float* dx) {
    if (dy == nullptr || y == nullptr || dx == nullptr || n < 0) return VB_E_BADARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(tanh_bwd_kernel, dim3(vb_grid_for(n, 256, 2048)), dim3(256), 0, static_cast<hipStream_t>(stream), (long)n,
                       dy, y, dx);
    VB_LAUNCH_CHECK();
    return 0;
}
