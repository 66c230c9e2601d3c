// BertLayerNorm (reference vilbert.py:313-317) forward and backward, on fp32 rows and on the bf16 rows of the bf16 training
// stream and of the MX inference stream. Row layout, row I/O per element type and the fp32 finish: rowops.h. Statistics, the
// normalisation and the gradient sums are fp32 everywhere - only what crosses HBM differs.
#include "rowops.h"
#include "rng.h"

using namespace vbrow;

namespace {

// ---- forward, fp32 rows: one row per wave; optionally also the row's e4m3 codes + scale, or its MX codes (ln_finish) ----
template <int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(long rows, int n_cols, const float* __restrict__ x,
                                                        const float* __restrict__ x2,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float eps,
                                                        float* __restrict__ y, float* mean, float* rstd,
                                                        unsigned char* __restrict__ q, long ldq,
                                                        float* __restrict__ qscale, unsigned* __restrict__ mxs,
                                                        long mxs_rows) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* xr = x + row * n_cols;
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (col < n_cols) {
            v[i] = *reinterpret_cast<const f32x4*>(xr + col);
            if (x2 != nullptr) v[i] += *reinterpret_cast<const f32x4*>(x2 + row * n_cols + col);
        }
    }
    ln_finish<NV>(v, n_cols, lane, gamma, beta, eps, y + row * n_cols, mean ? mean + row : nullptr,
                  rstd ? rstd + row : nullptr, nullptr, q ? q + row * ldq : nullptr, (q && qscale) ? qscale + row : nullptr,
                  mxs ? mxs + row : nullptr, mxs_rows);
}

// ---- forward, bf16 rows ----
// A wave owns R consecutive rows and runs their dependent chains (load -> sum -> wave reduction -> squared deviations -> wave
// reduction -> store) side by side: with one row per wave the launch is bound by that chain's latency and the number of block
// rounds, not by HBM (11.4 us for 28 MB at 9,216 x 768: 2,304 blocks for the 2,048 places of the chip; the MX form 29.5 us
// for 70 MB at 18,432 x 768). The rows stay PACKED in registers between the phases (2 registers per 4 values, widened where
// used): four rows of 1,024 columns in 32 registers keep the occupancy at 8 waves per SIMD (as fp32 they took 64 and the
// MX form 112).
// Emit = what leaves besides the bf16 row: the statistics (training), or the row's MX codes (mx8.h; MX inference).
struct EmitStats {
    static constexpr bool MX = false;
    float* __restrict__ mean;   // (either may be null)
    float* __restrict__ rstd;
};
struct EmitMX {
    static constexpr bool MX = true;
    unsigned char* __restrict__ q;
    long ldq;
    unsigned* __restrict__ mxs;   // scale plane base, plane stride mxs_rows words
    long mxs_rows;
};

// the normalised values of a lane's 4 columns of one resident row
__device__ __forceinline__ f32x4 ln16_value(const uint2 w, const f32x4 g, const f32x4 b, float mean, float rstd) {
    return g * ((RowBF16::unpack(w) - mean) * rstd) + b;
}

template <int NV, int R, typename Emit>
__global__ __launch_bounds__(256) void layernorm16_kernel(long rows, int n_cols, const unsigned short* __restrict__ x,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          float eps, unsigned short* __restrict__ y, const Emit out) {
    using IO = RowBF16;
    const int lane = threadIdx.x & 63;
    const long row0 = ((long)blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6)) * R;
    if (row0 >= rows) return;
    long rrow[R];                                       // rows past the end: row0 again, every store masked
    bool have[R];                                       // (wave-uniform)
#pragma unroll
    for (int r = 0; r < R; ++r) {
        have[r] = row0 + r < rows;
        rrow[r] = have[r] ? row0 + r : row0;
    }
    uint2 w[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            w[r][i] = uint2{0u, 0u};
            if (col < n_cols) w[r][i] = *reinterpret_cast<const uint2*>(x + rrow[r] * n_cols + col);
        }
    auto opaque = [&]() {   // the compiler must not keep the widened copies of one phase alive for the next
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < NV; ++i) asm volatile("" : "+v"(w[r][i].x), "+v"(w[r][i].y));
    };
    float mu[R], q[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        mu[r] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const f32x4 v = IO::unpack(w[r][i]);
            mu[r] += (v[0] + v[1]) + (v[2] + v[3]);     // (columns past n_cols hold 0)
        }
    }
    wave_sum_rows(mu);
    if (R > 1) opaque();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        mu[r] /= (float)n_cols;
        q[r] = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            if (col < n_cols) {
                const f32x4 d = IO::unpack(w[r][i]) - mu[r];
                q[r] += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
            }
        }
    }
    wave_sum_rows(q);
    if (R > 1) opaque();
    if constexpr (!Emit::MX) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            q[r] = 1.0f / sqrtf(q[r] / (float)n_cols + eps);
            if (lane == 0 && have[r]) {
                if (out.mean != nullptr) out.mean[rrow[r]] = mu[r];
                if (out.rstd != nullptr) out.rstd[rrow[r]] = q[r];
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            if (col < n_cols) {
                const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + col), b = *reinterpret_cast<const f32x4*>(beta + col);
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (have[r]) IO::store(y + rrow[r] * n_cols + col, ln16_value(w[r][i], g, b, mu[r], q[r]));
            }
        }
    } else {
        // the cross-lane steps inside mx_quant_chunk run for every lane: columns past the row and rows that do not exist go
        // through with their stores masked
        const int nkt = n_cols >> 7;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            const bool ok = col < n_cols;
            f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f}, b = f32x4{0.f, 0.f, 0.f, 0.f};
            if (ok) {
                g = *reinterpret_cast<const f32x4*>(gamma + col);
                b = *reinterpret_cast<const f32x4*>(beta + col);
            }
            const int kt = 2 * i + (lane >> 5);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float rstd = 1.0f / sqrtf(q[r] / (float)n_cols + eps);
                const bool live = ok && have[r];
                f32x4 v = IO::unpack(w[r][i]);
                if (ok) v = ln16_value(w[r][i], g, b, mu[r], rstd);
                if (live) IO::store(y + rrow[r] * n_cols + col, v);
                mx_quant_chunk(v, live, lane, have[r] ? kt : nkt, nkt,
                               reinterpret_cast<unsigned*>(out.q + rrow[r] * out.ldq + (ok ? col : 0)),
                               out.mxs + (long)(kt < nkt ? kt : 0) * out.mxs_rows + rrow[r]);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LayerNorm backward. Per row (xhat = (x - mean) rstd, g = dy * gamma):
//   dx = rstd * (g - mean(g) - xhat * mean(g * xhat))
//   dgamma = sum_rows dy * xhat,  dbeta = sum_rows dy
// Stage 1: one wave walks LNB_ROWS_PER_WAVE rows keeping its column partials of dgamma / dbeta in registers; the four
// waves of a block combine theirs through LDS (rows of <= 1024 columns) and write ONE workspace row per block, wider rows
// one per wave; stage 2 sums the workspace rows column-wise. No atomics: the result is deterministic.
// ------------------------------------------------------------------------------------------------
constexpr int LNB_ROWS_PER_WAVE = 4;   // few rows per wave: 9216 rows -> 2304 waves keep the chip's 1024 SIMDs busy
constexpr int LNB_ROWS_PER_BLOCK = 4 * LNB_ROWS_PER_WAVE;

inline long lnb_blocks(long rows) { return (rows + LNB_ROWS_PER_BLOCK - 1) / LNB_ROWS_PER_BLOCK; }

template <int NV, typename IO>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(long rows, int n_cols, const typename IO::elem* __restrict__ dy,
                                                            const typename IO::elem* __restrict__ x,
                                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            typename IO::elem* __restrict__ dx, float* __restrict__ ws,
                                                            typename IO::elem* __restrict__ dxd, float drop_p,
                                                            float drop_scale, uint64_t seed_in,
                                                            const uint64_t* __restrict__ epoch) {
    // dxd (optional): dx under the dropout mask of the dense layer in FRONT of this LayerNorm (the gradient that layer's
    // backward GEMMs consume), written in the same pass (saves the separate vb_dropout launch over dx) - element index =
    // row * n_cols + col as in that layer's forward epilogue
    const uint64_t seed = dxd != nullptr ? vb_seed_with_epoch(seed_in, epoch) : 0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long part = (long)blockIdx.x * 4 + wave;
    const long row_begin = part * LNB_ROWS_PER_WAVE;
    f32x4 gam[NV], dg[NV], db[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        gam[i] = col < n_cols ? *reinterpret_cast<const f32x4*>(gamma + col) : f32x4{0.f, 0.f, 0.f, 0.f};
        dg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        db[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    // IO::PREFETCH (bf16 rows): the NEXT row's dy / x (packed) and statistics are requested before this row's two wave
    // reductions: a wave's four rows were four strictly sequential load -> reduce -> store chains (23.8 us for 42 MB at
    // 9,216 x 768). Not for fp32 rows, which go up to NV = 16: the 2 NV extra live vectors would cost occupancy there.
    [[maybe_unused]] typename IO::packed ndy[NV], nx[NV];
    [[maybe_unused]] float nmu = 0.f, nrs = 0.f;
    [[maybe_unused]] auto fetch = [&](long row) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            ndy[i] = IO::zero();
            nx[i] = IO::zero();
            if (col < n_cols) {
                ndy[i] = *reinterpret_cast<const typename IO::packed*>(dy + row * n_cols + col);
                nx[i] = *reinterpret_cast<const typename IO::packed*>(x + row * n_cols + col);
            }
        }
        nmu = mean[row];
        nrs = rstd[row];
    };
    if constexpr (IO::PREFETCH)
        if (row_begin < rows) fetch(row_begin);
    for (int rr = 0; rr < LNB_ROWS_PER_WAVE; ++rr) {
        const long row = row_begin + rr;
        if (row >= rows) break;
        const float mu = IO::PREFETCH ? nmu : mean[row], rs = IO::PREFETCH ? nrs : rstd[row];
        f32x4 xh[NV], g[NV];
        [[maybe_unused]] f32x4 dcur[NV];   // (bf16 rows: the prefetched dy, widened)
        if constexpr (IO::PREFETCH) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                dcur[i] = IO::unpack(ndy[i]);
                xh[i] = IO::unpack(nx[i]);
            }
            if (rr + 1 < LNB_ROWS_PER_WAVE && row + 1 < rows) fetch(row + 1);
        }
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = VB_LANE_COL(i, lane);
            if constexpr (!IO::PREFETCH) xh[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            g[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (col < n_cols) {
                // (fp32 rows: each chunk is loaded here, where it is used)
                const f32x4 d = IO::PREFETCH ? dcur[i] : *reinterpret_cast<const f32x4*>(dy + row * n_cols + col);
                xh[i] = ((IO::PREFETCH ? xh[i] : *reinterpret_cast<const f32x4*>(x + row * n_cols + col)) - mu) * rs;
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
            if (col < n_cols) {
                const f32x4 d = (g[i] - m1 - xh[i] * m2) * rs;
                IO::store(dx + row * n_cols + col, d);
                if (dxd != nullptr) {
                    f32x4 dd;
                    const uint64_t idx = (uint64_t)(row * n_cols + col);
#pragma unroll
                    for (int e = 0; e < 4; ++e) dd[e] = vb_keep(seed, idx + e, drop_p) ? d[e] * drop_scale : 0.f;
                    IO::store(dxd + row * n_cols + col, dd);
                }
            }
        }
    }
    constexpr bool BLOCK_REDUCE = NV <= 4;
    __shared__ f32x4 red[BLOCK_REDUCE ? 3 * 2 * NV * 64 : 1];
    if (BLOCK_REDUCE) {
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
    }
    float* w = ws + (BLOCK_REDUCE ? (long)blockIdx.x : part) * 2 * n_cols;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int col = VB_LANE_COL(i, lane);
        if (col < n_cols) {
            *reinterpret_cast<f32x4*>(w + col) = dg[i];
            *reinterpret_cast<f32x4*>(w + n_cols + col) = db[i];
        }
    }
}

// Rows wider than 4096 columns (nothing in the two-stream models; the C ABI allows up to VB_MAX_LN_COLS): one wave per
// row, the row walked twice in 256-column chunks (pass 1: the two row means, pass 2: dx and this row's dgamma / dbeta
// terms, written straight to the workspace: one partial per row) - no per-column accumulators in registers, so no
// scratch (the register-resident variant above spilled 940 bytes per lane at NV = 32).
__global__ __launch_bounds__(256) void layernorm_bwd_wide_kernel(long rows, int n_cols, const float* __restrict__ dy,
                                                                 const float* __restrict__ x,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd,
                                                                 const float* __restrict__ gamma,
                                                                 float* __restrict__ dx, float* __restrict__ ws) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float mu = mean[row], rs = rstd[row];
    const float* __restrict__ dyr = dy + row * n_cols;
    const float* __restrict__ xr = x + row * n_cols;
    float s1 = 0.f, s2 = 0.f;
    for (int col = lane * 4; col < n_cols; col += 256) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(dyr + col);
        const f32x4 xh = (*reinterpret_cast<const f32x4*>(xr + col) - mu) * rs;
        const f32x4 g = d * *reinterpret_cast<const f32x4*>(gamma + col);
        s1 += (g[0] + g[1]) + (g[2] + g[3]);
        s2 += (g[0] * xh[0] + g[1] * xh[1]) + (g[2] * xh[2] + g[3] * xh[3]);
    }
    const float m1 = wave_sum(s1) / (float)n_cols, m2 = wave_sum(s2) / (float)n_cols;
    float* __restrict__ w = ws + row * 2 * n_cols;
    for (int col = lane * 4; col < n_cols; col += 256) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(dyr + col);
        const f32x4 xh = (*reinterpret_cast<const f32x4*>(xr + col) - mu) * rs;
        const f32x4 g = d * *reinterpret_cast<const f32x4*>(gamma + col);
        *reinterpret_cast<f32x4*>(dx + row * n_cols + col) = (g - m1 - xh * m2) * rs;
        *reinterpret_cast<f32x4*>(w + col) = d * xh;
        *reinterpret_cast<f32x4*>(w + n_cols + col) = d;
    }
}

// Stage 2: column sums of `parts` workspace rows of width 2 * n_cols -> [dgamma | dbeta]. Block = 1024 threads = 16 row
// groups x 64 columns; each group strides over the parts with INFLIGHT independent partial sums (= loads in flight per
// thread; INFLIGHT = 1 is the plain running sum), then the 16 groups are added in order through LDS. The summation order
// is part of each caller's result bits: the fp32 rows use <1>, the bf16 rows <4>.
template <int INFLIGHT>
__global__ __launch_bounds__(1024) void colreduce_kernel(long parts, int width, const float* __restrict__ ws,
                                                         float* __restrict__ out0, float* __restrict__ out1, int n_cols) {
    static_assert(INFLIGHT == 1 || INFLIGHT == 4, "instantiated forms");
    __shared__ float red[16][INFLIGHT == 1 ? 64 : 65];
    const int c = threadIdx.x & 63, pg = threadIdx.x >> 6;
    const int col = blockIdx.x * 64 + c;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (col < width) {
        long p = pg;
        if constexpr (INFLIGHT == 4)
            for (; p + 48 < parts; p += 64) {
                s0 += ws[p * width + col];
                s1 += ws[(p + 16) * width + col];
                s2 += ws[(p + 32) * width + col];
                s3 += ws[(p + 48) * width + col];
            }
        for (; p < parts; p += 16) s0 += ws[p * width + col];
    }
    red[pg][c] = INFLIGHT == 4 ? (s0 + s1) + (s2 + s3) : s0;
    __syncthreads();
    if (pg == 0 && col < width) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[i][c];
        if (col < n_cols) out0[col] = t;
        else out1[col - n_cols] = t;
    }
}

template <int INFLIGHT>
int launch_colreduce(hipStream_t st, long parts, int n_cols, const float* ws, float* dgamma, float* dbeta) {
    const int width = 2 * n_cols;
    hipLaunchKernelGGL(colreduce_kernel<INFLIGHT>, dim3((unsigned)((width + 63) / 64)), dim3(1024), 0, st, parts, width, ws,
                       dgamma, dbeta, n_cols);
    VB_LAUNCH_CHECK();
    return 0;
}

// the codes target of the emitting forwards: row stride ldq bytes, written as 4-byte words
inline bool codes_ok(const void* q, int64_t ldq, int n_cols) { return ldq >= n_cols && ldq % 4 == 0 && all_aligned(4, {q}); }

// the three fp32 forwards: plain (q null), + e4m3 codes and scale (q, qscale), + MX codes (q, mxs)
int launch_layernorm(void* stream, int64_t rows, int32_t n_cols, const float* x, const float* x2, const float* gamma,
                     const float* beta, float eps, float* y, float* mean, float* rstd, uint8_t* q, int64_t ldq,
                     float* qscale, uint32_t* mxs, int64_t mxs_rows) {
    if (!all_aligned(16, {x, x2, y, gamma, beta}) || (q != nullptr && !codes_ok(q, ldq, n_cols)) || !all_aligned(4, {mxs}))
        return VB_E_ALIGN;
    const dim3 grid((unsigned)((rows + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK)), block(256);
    dispatch_nv<32>(nv_for(n_cols), [&](auto nv) {
        hipLaunchKernelGGL((layernorm_kernel<decltype(nv)::value>), grid, block, 0, static_cast<hipStream_t>(stream), (long)rows,
                           n_cols, x, x2, gamma, beta, eps, y, mean, rstd, q, (long)ldq, qscale, mxs, (long)mxs_rows);
    });
    VB_LAUNCH_CHECK();
    return 0;
}

// rows x NV x Emit of the bf16 forward: R rows per wave, NV up to MAX
template <int R, int MAX, typename Emit>
void launch_layernorm16(void* stream, int64_t rows, int32_t n_cols, const uint16_t* x, const float* gamma, const float* beta,
                        float eps, uint16_t* y, const Emit out) {
    const dim3 grid((unsigned)((rows + R * ROWS_PER_BLOCK - 1) / (R * ROWS_PER_BLOCK))), block(256);
    dispatch_nv<MAX>(nv_for(n_cols), [&](auto nv) {
        hipLaunchKernelGGL((layernorm16_kernel<decltype(nv)::value, R, Emit>), grid, block, 0, static_cast<hipStream_t>(stream),
                           (long)rows, n_cols, x, gamma, beta, eps, y, out);
    });
}

// the checks common to both backwards, then stage 1 (NV <= MAX) and the column reduce
template <typename IO, int MAX, int INFLIGHT>
int layernorm_bwd_impl(void* stream, int64_t rows, int32_t n_cols, const typename IO::elem* dy, const typename IO::elem* x,
                       const float* mean, const float* rstd, const float* gamma, typename IO::elem* dx, float* dgamma,
                       float* dbeta, float* workspace, typename IO::elem* dxd, float drop_p, uint64_t seed) {
    if (!all_aligned(IO::ALIGN, {dy, x, dx, dxd}) || !all_aligned(16, {gamma, workspace})) return VB_E_ALIGN;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long blocks = lnb_blocks(rows);
    const float dscale = dxd != nullptr ? 1.0f / (1.0f - drop_p) : 1.0f;
    const uint64_t* epoch = vb_seed_epoch();   // (read by the kernel only with dxd)
    dispatch_nv<MAX>(nv_for(n_cols), [&](auto nv) {
        hipLaunchKernelGGL((layernorm_bwd_kernel<decltype(nv)::value, IO>), dim3((unsigned)blocks), dim3(256), 0, st, (long)rows,
                           n_cols, dy, x, mean, rstd, gamma, dx, workspace, dxd, drop_p, dscale, seed, epoch);
    });
    VB_LAUNCH_CHECK();
    return launch_colreduce<INFLIGHT>(st, nv_for(n_cols) <= 4 ? blocks : blocks * 4, n_cols, workspace, dgamma, dbeta);
}

int layernorm_bwd_f32(void* stream, int64_t rows, int32_t n_cols, const float* dy, const float* x, const float* mean,
                      const float* rstd, const float* gamma, float* dx, float* dgamma, float* dbeta, float* workspace,
                      float* dxd, float drop_p, uint64_t seed) {
    if (any_null({dy, x, mean, rstd, gamma, dx, dgamma, dbeta, workspace}) || rows <= 0) return VB_E_BADARG;
    if (int e = check_cols(n_cols)) return e;
    if (nv_for(n_cols) <= 16)
        return layernorm_bwd_impl<RowF32, 16, 1>(stream, rows, n_cols, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, workspace,
                                                 dxd, drop_p, seed);
    if (!all_aligned(16, {dy, x, dx, gamma, workspace})) return VB_E_ALIGN;
    if (dxd != nullptr) return VB_E_RANGE;    // (the fused mask is not offered for rows wider than 4096)
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(layernorm_bwd_wide_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (long)rows, n_cols, dy, x,
                       mean, rstd, gamma, dx, workspace);
    VB_LAUNCH_CHECK();
    return launch_colreduce<1>(st, rows, n_cols, workspace, dgamma, dbeta);
}

}  // namespace

extern "C" int vb_layernorm_fwd(void* stream, int64_t rows, int32_t n_cols, const float* x, const float* x2,
                                const float* gamma, const float* beta, float eps, float* y, float* mean,
                                float* rstd) {
    if (any_null({x, gamma, beta, y}) || rows <= 0) return VB_E_BADARG;
    if (int e = check_cols(n_cols)) return e;
    return launch_layernorm(stream, rows, n_cols, x, x2, gamma, beta, eps, y, mean, rstd, nullptr, 0, nullptr, nullptr, 0);
}

// LayerNorm forward that also emits the row's e4m3 codes + scale (inference in fp8 mode: the consumer GEMMs read the
// codes, the fp32 row stays for the residual path). Bit-identical to vb_layernorm_fwd followed by vb_quantize_rows_fp8.
extern "C" int vb_layernorm_fwd_fp8(void* stream, int64_t rows, int32_t n_cols, const float* x, const float* x2,
                                    const float* gamma, const float* beta, float eps, float* y, uint8_t* q,
                                    int64_t ldq, float* qscale) {
    if (any_null({x, gamma, beta, y, q, qscale}) || rows <= 0) return VB_E_BADARG;
    if (int e = check_cols(n_cols)) return e;
    return launch_layernorm(stream, rows, n_cols, x, x2, gamma, beta, eps, y, nullptr, nullptr, q, ldq, qscale, nullptr, 0);
}

// LayerNorm forward that also emits its output rows in the MX e4m3 format (mx8.hip) for the linears consuming it; the
// fp32 row stays for the residual path. Bit-identical to vb_layernorm_fwd followed by vb_quantize_rows_mx on y.
extern "C" int vb_layernorm_fwd_mx(void* stream, int64_t rows, int32_t n_cols, const float* x, const float* x2,
                                   const float* gamma, const float* beta, float eps, float* y, uint8_t* q, int64_t ldq,
                                   uint32_t* scales, int64_t scale_rows) {
    if (any_null({x, gamma, beta, y, q, scales}) || rows <= 0) return VB_E_BADARG;
    if (int e = check_cols(n_cols)) return e;
    if (n_cols % 128 != 0 || scale_rows < rows) return VB_E_RANGE;
    return launch_layernorm(stream, rows, n_cols, x, x2, gamma, beta, eps, y, nullptr, nullptr, q, ldq, nullptr, scales,
                            scale_rows);
}

// LayerNorm of the MX path's bf16 residual stream: bf16 row in, bf16 row + MX codes out
extern "C" int vb_layernorm_fwd_mx16(void* stream, int64_t rows, int32_t n_cols, const uint16_t* x, const float* gamma,
                                     const float* beta, float eps, uint16_t* y, uint8_t* q, int64_t ldq, uint32_t* scales,
                                     int64_t scale_rows) {
    if (any_null({x, gamma, beta, y, q, scales}) || rows <= 0) return VB_E_BADARG;
    if (int e = check_cols(n_cols)) return e;
    if (n_cols % 128 != 0 || scale_rows < rows) return VB_E_RANGE;
    if (!all_aligned(RowBF16::ALIGN, {x, y}) || !all_aligned(16, {gamma, beta}) || !codes_ok(q, ldq, n_cols) ||
        !all_aligned(4, {scales}))
        return VB_E_ALIGN;
    const EmitMX out{q, (long)ldq, scales, (long)scale_rows};
    // rows per wave: 2, or 4 when two rows per wave would need more blocks than fit the chip at once (8 per CU) - at batch
    // 512 (18,432 rows) the 2,304 blocks of the two-row form ran as one full round plus a 12 % tail round of the same
    // latency. Four only for rows of at most 1,024 columns (4 x 4 packed register pairs per lane).
    if ((rows + 2 * ROWS_PER_BLOCK - 1) / (2 * ROWS_PER_BLOCK) <= 2048 || n_cols > 1024)
        launch_layernorm16<2, 32>(stream, rows, n_cols, x, gamma, beta, eps, y, out);
    else
        launch_layernorm16<4, 4>(stream, rows, n_cols, x, gamma, beta, eps, y, out);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int vb_layernorm_fwd_bf16(void* stream, int64_t rows, int32_t n_cols, const uint16_t* x, const float* gamma,
                                     const float* beta, float eps, uint16_t* y, float* mean, float* rstd) {
    if (any_null({x, gamma, beta, y}) || rows <= 0) return VB_E_BADARG;
    if (n_cols <= 0 || n_cols % 4 != 0 || n_cols > 1024) return VB_E_RANGE;
    if (!all_aligned(RowBF16::ALIGN, {x, y}) || !all_aligned(16, {gamma, beta})) return VB_E_ALIGN;
    const EmitStats out{mean, rstd};
    // rows per wave: 1 for small launches (more blocks than rows / 8 would leave CUs idle), else the smallest of 2 / 4 whose
    // blocks fit the chip in one round (8 blocks of 4 waves per CU)
    if (rows < 4096) launch_layernorm16<1, 4>(stream, rows, n_cols, x, gamma, beta, eps, y, out);
    else if ((rows + 7) / 8 <= 2048) launch_layernorm16<2, 4>(stream, rows, n_cols, x, gamma, beta, eps, y, out);
    else launch_layernorm16<4, 4>(stream, rows, n_cols, x, gamma, beta, eps, y, out);
    VB_LAUNCH_CHECK();
    return 0;
}

extern "C" int64_t vb_layernorm_bwd_workspace(int64_t rows, int32_t n_cols) {
    if (rows <= 0 || n_cols <= 0) return 0;
    if (nv_for(n_cols) > 16) return rows * 2 * n_cols;   // wide rows: one partial per row (layernorm_bwd_wide_kernel)
    const int64_t parts = (rows + LNB_ROWS_PER_WAVE - 1) / LNB_ROWS_PER_WAVE;
    const int64_t parts_padded = (parts + 3) / 4 * 4;  // whole blocks write
    return parts_padded * 2 * n_cols;
}

extern "C" int vb_layernorm_bwd(void* stream, int64_t rows, int32_t n_cols, const float* dy, const float* x,
                                const float* mean, const float* rstd, const float* gamma, float* dx,
                                float* dgamma, float* dbeta, float* workspace) {
    return layernorm_bwd_f32(stream, rows, n_cols, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, workspace, nullptr, 0.f, 0);
}

extern "C" int vb_layernorm_bwd_drop(void* stream, int64_t rows, int32_t n_cols, const float* dy, const float* x,
                                     const float* mean, const float* rstd, const float* gamma, float* dx,
                                     float* dgamma, float* dbeta, float* workspace, float* dx_dropped, float dropout_p,
                                     uint64_t seed) {
    if (dx_dropped == nullptr || !(dropout_p > 0.f && dropout_p < 1.f)) return VB_E_BADARG;
    if (!vb_aligned16(dx_dropped)) return VB_E_ALIGN;
    return layernorm_bwd_f32(stream, rows, n_cols, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, workspace, dx_dropped,
                             dropout_p, seed);
}

extern "C" int64_t vb_layernorm_bwd_bf16_workspace(int64_t rows, int32_t n_cols) {
    return lnb_blocks(rows) * 2 * (int64_t)n_cols;   // one partial per block (rows of at most 1,024 columns)
}

extern "C" int vb_layernorm_bwd_bf16(void* stream, int64_t rows, int32_t n_cols, const uint16_t* dy, const uint16_t* x,
                                     const float* mean, const float* rstd, const float* gamma, uint16_t* dx, float* dgamma,
                                     float* dbeta, float* workspace, uint16_t* dx_dropped, float dropout_p, uint64_t seed) {
    if (any_null({dy, x, mean, rstd, gamma, dx, dgamma, dbeta, workspace}) || rows <= 0) return VB_E_BADARG;
    if (n_cols <= 0 || n_cols % 4 != 0 || n_cols > 1024) return VB_E_RANGE;
    if (dx_dropped != nullptr && !(dropout_p > 0.f && dropout_p < 1.f)) return VB_E_BADARG;
    return layernorm_bwd_impl<RowBF16, 4, 4>(stream, rows, n_cols, dy, x, mean, rstd, gamma, dx, dgamma, dbeta, workspace,
                                             dx_dropped, dropout_p, seed);
}
