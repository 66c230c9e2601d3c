// Ordered text-embedding backward: vb_text_embed_bwd with the deterministic setting on (vb_set_deterministic).
//
// The four gradient tables are one keyed reduction over the rows r = b * n_out + t_out of dx. Every row yields up to
// three entries, each with a key in one combined key space:
//   word      key = id                                 (0 < id < vocab; row 0 is the padding row)
//   position  key = vocab + t                          (every row but the task-token row)
//   type      key = vocab + n_tok + type               (0 <= type < n_types; a one-row table has no type 1)
//   task      key = vocab + n_tok + n_types + task     (the task-token row t_out = 1, 0 <= task < n_tasks)
// Skipped entries get the sentinel key vocab + n_tok + n_types + n_tasks. A key's rows are visited in ascending r, cut
// into consecutive runs of EMB_RUN rows, each run summed left to right in fp32, the run sums added left to right, and
// the total applied to the table row with ONE add (row = row + total). Nothing depends on the order blocks run in:
//   1. a stable LSD radix sort of the entries by key (2 passes of 9 bits; per-tile digit counts, one exclusive scan,
//      a scatter whose in-tile ranks come from wave ballots) - entries are enumerated slot-major (e = slot * rows + r),
//      so equal keys stay in ascending r;
//   2. segment bounds of every present key in the sorted list;
//   3. one wave per tile of EMB_RUN sorted positions (and per 256-column slice) sums the runs that START in its tile
//      (at most 2 x EMB_RUN rows per wave, so a hot key spreads over as many waves as it has runs): a key with a single
//      run updates its table row directly, a longer key parks each run sum in one of two slots of the tile (at most
//      one full-length run and one short last run of such keys start in a tile);
//   4. one wave per tile whose first position starts a multi-run key adds that key's run sums in run order.
// Scratch: the (device, stream) slice of the deterministic workspace; nothing is allocated, no memset, no host sync, all
// grid sizes follow from the call's arguments (capture-safe).
#include "common.h"
#include "det_workspace.h"

namespace {

constexpr int EMB_RUN = 64;                 // rows per run (= one wave lane per sorted position of a tile)
constexpr int SORT_BITS = 9;
constexpr int SORT_BUCKETS = 1 << SORT_BITS;
constexpr int SORT_TILE = 1024;             // entries per sort block: 4 waves x 4 rounds of 64
constexpr int EMB_MAX_KEYS = 1 << (2 * SORT_BITS);
constexpr int EMB_BATCH = 16;               // independent row loads in flight per lane before the ordered adds

struct EmbKeys {
    int n_tok, n_out, rows, vocab, n_types, n_tasks;
    int key_pos, key_type, key_task, key_end;
    const int64_t* ids;
    const int64_t* seg;
    const int64_t* task_ids;
    bool skip_pos0, skip_type0;   // the baseline's padding rows (vbb_text_embed_bwd): position 0 / type 0 yield no entry
};

struct EmbTables {
    float* dword;
    float* dpos;
    float* dtype;
    float* dtask;
    int key_pos, key_type, key_task, key_end;
};

// key of entry e (slot-major: e = slot * rows + r; slot 0 = word or task, 1 = position, 2 = type); *row = r
__device__ __forceinline__ int entry_key(const EmbKeys& k, int e, int* row) {
    const int slot = e / k.rows, r = e - slot * k.rows;
    *row = r;
    const int b = r / k.n_out, t_out = r - b * k.n_out;
    const bool has_task = k.task_ids != nullptr;
    if (has_task && t_out == 1) {           // the task-token row has no word, position or type
        if (slot != 0) return k.key_end;
        const int64_t task = k.task_ids[b];
        return (task >= 0 && task < k.n_tasks) ? k.key_task + (int)task : k.key_end;
    }
    const int t = (has_task && t_out >= 2) ? t_out - 1 : t_out;
    if (slot == 1) return (k.skip_pos0 && t == 0) ? k.key_end : k.key_pos + t;
    if (slot == 0) {
        const int64_t id = k.ids[(long)b * k.n_tok + t];
        return (id > 0 && id < k.vocab) ? (int)id : k.key_end;
    }
    const int64_t ty = k.seg[(long)b * k.n_tok + t];
    if (k.skip_type0 && ty == 0) return k.key_end;
    return (ty >= 0 && ty < k.n_types) ? k.key_type + (int)ty : k.key_end;
}

// digit counts of one tile of SORT_TILE entries: hist[digit * nblk + tile] (digit-major, so one exclusive scan of the
// whole array gives every (digit, tile) its first output position)
template <bool FIRST>
__global__ __launch_bounds__(256) void emb_sort_hist_kernel(EmbKeys k, int n, const int* __restrict__ keys_in, int shift,
                                                            int* __restrict__ hist, int nblk) {
    __shared__ int cnt[SORT_BUCKETS];
    for (int d = threadIdx.x; d < SORT_BUCKETS; d += 256) cnt[d] = 0;
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = (long)blockIdx.x * SORT_TILE + q * 256 + threadIdx.x;
        if (i < n) {
            int r;
            const int key = FIRST ? entry_key(k, (int)i, &r) : keys_in[i];
            atomicAdd(&cnt[(key >> shift) & (SORT_BUCKETS - 1)], 1);
        }
    }
    __syncthreads();
    for (int d = threadIdx.x; d < SORT_BUCKETS; d += 256) hist[(long)d * nblk + blockIdx.x] = cnt[d];
}

// exclusive scan of n ints in place, one block: contiguous chunk per thread, Hillis-Steele over the chunk sums
__global__ __launch_bounds__(1024) void emb_sort_scan_kernel(int* __restrict__ h, int n) {
    __shared__ int part[1024];
    const int per = (n + 1023) / 1024;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += h[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        const int v = h[i];
        h[i] = run;
        run += v;
    }
}

// stable scatter of one tile by the digit at `shift`: wave w owns entries [w * 256, w * 256 + 256) of the tile in four
// rounds of 64; within a round a lane's rank among the lanes of its digit comes from SORT_BITS ballots
template <bool FIRST>
__global__ __launch_bounds__(256) void emb_sort_scatter_kernel(EmbKeys k, int n, const int* __restrict__ keys_in,
                                                               const int* __restrict__ vals_in, int shift,
                                                               const int* __restrict__ offs, int nblk,
                                                               int* __restrict__ keys_out, int* __restrict__ vals_out) {
    __shared__ int cnt[4][SORT_BUCKETS];
    for (int j = threadIdx.x; j < 4 * SORT_BUCKETS; j += 256) cnt[j / SORT_BUCKETS][j % SORT_BUCKETS] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint64_t below = (1ull << lane) - 1;
    int key[4], val[4], rank[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = (long)blockIdx.x * SORT_TILE + w * 256 + q * 64 + lane;
        const bool ok = i < n;
        key[q] = 0;
        val[q] = 0;
        if (ok) {
            if (FIRST) key[q] = entry_key(k, (int)i, &val[q]);
            else {
                key[q] = keys_in[i];
                val[q] = vals_in[i];
            }
        }
        const int d = (key[q] >> shift) & (SORT_BUCKETS - 1);
        uint64_t peers = __ballot(ok);
#pragma unroll
        for (int bit = 0; bit < SORT_BITS; ++bit) {
            const uint64_t m = __ballot((d >> bit) & 1);
            peers &= ((d >> bit) & 1) ? m : ~m;
        }
        const int base = ok ? cnt[w][d] : 0;
        rank[q] = base + __popcll(peers & below);
        // the highest lane of a digit advances the wave's count (after every lane of the wave has read it)
        if (ok && (peers >> lane) == 1ull) cnt[w][d] = base + __popcll(peers);
    }
    __syncthreads();
    for (int d = threadIdx.x; d < SORT_BUCKETS; d += 256) {
        int run = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int c = cnt[v][d];
            cnt[v][d] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const long i = (long)blockIdx.x * SORT_TILE + w * 256 + q * 64 + lane;
        if (i < n) {
            const int d = (key[q] >> shift) & (SORT_BUCKETS - 1);
            const long pos = (long)offs[(long)d * nblk + blockIdx.x] + cnt[w][d] + rank[q];
            if (pos >= 0 && pos < n) {
                keys_out[pos] = key[q];
                vals_out[pos] = val[q];
            }
        }
    }
}

// [seg_start[k], seg_end[k]) = the sorted positions of key k (written for the keys present only)
__global__ __launch_bounds__(256) void emb_bounds_kernel(int n, int key_end, const int* __restrict__ skey,
                                                         int* __restrict__ seg_start, int* __restrict__ seg_end) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = skey[i];
    if (k < 0 || k >= key_end) return;
    if (i == 0 || skey[i - 1] != k) seg_start[k] = (int)i;
    if (i == n - 1 || skey[i + 1] != k) seg_end[k] = (int)i + 1;
}

__device__ __forceinline__ float* table_row(const EmbTables& t, int k, int hidden) {
    if (k < t.key_pos) return t.dword + (long)k * hidden;
    if (k < t.key_type) return t.dpos + (long)(k - t.key_pos) * hidden;
    if (k < t.key_task) return t.dtype + (long)(k - t.key_type) * hidden;
    return t.dtask + (long)(k - t.key_task) * hidden;
}

// row = row + total (element stores: the tables carry no alignment promise)
__device__ __forceinline__ void row_add(float* row, int col, f32x4 v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) row[col + e] = row[col + e] + v[e];
}

// one wave per (tile of EMB_RUN sorted positions, 256-column slice): the runs that start in the tile, each summed left
// to right; single-run keys finish here, the runs of longer keys go to part[(2 tile + full) * hidden]
__global__ __launch_bounds__(256) void emb_run_kernel(int n, int hidden, const int* __restrict__ skey,
                                                      const int* __restrict__ srow, const int* __restrict__ seg_start,
                                                      const int* __restrict__ seg_end, const float* __restrict__ dx,
                                                      float* __restrict__ part, EmbTables tb) {
    const int lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long i = tile * EMB_RUN + lane;
    const int col = blockIdx.y * 256 + lane * 4;
    int k = tb.key_end, s = 0;
    if (i < n) k = skey[i];
    bool starts = false;
    if (k >= 0 && k < tb.key_end) {
        s = seg_start[k];
        starts = (i - s) % EMB_RUN == 0;
    }
    uint64_t m = __ballot(starts);
    while (m != 0) {
        const int L = __ffsll((unsigned long long)m) - 1;
        m &= m - 1;
        const int p = (int)(tile * EMB_RUN) + L;
        const int kk = __shfl(k, L), ss = __shfl(s, L);
        const int e = seg_end[kk];
        const int len = min(EMB_RUN, e - p);
        const int myrow = lane < len ? srow[p + lane] : 0;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < len; j += EMB_BATCH) {
            f32x4 v[EMB_BATCH];
#pragma unroll
            for (int u = 0; u < EMB_BATCH; ++u) {
                const int r = __shfl(myrow, (j + u) & 63);
                v[u] = (j + u < len && col < hidden) ? *reinterpret_cast<const f32x4*>(dx + (long)r * hidden + col)
                                                     : acc;
            }
#pragma unroll
            for (int u = 0; u < EMB_BATCH; ++u)
                if (j + u < len) acc = (j + u == 0) ? v[u] : acc + v[u];
        }
        if (col < hidden) {
            if (e - ss <= EMB_RUN) row_add(table_row(tb, kk, hidden), col, acc);
            else *reinterpret_cast<f32x4*>(part + (2 * tile + (len == EMB_RUN ? 1 : 0)) * hidden + col) = acc;
        }
    }
}

// one wave per (tile, slice) whose tile holds the first position of a key with more than EMB_RUN rows (at most one:
// such a key runs past the tile): the key's run sums in run order, then one add into the table row
__global__ __launch_bounds__(256) void emb_combine_kernel(int n, int hidden, const int* __restrict__ skey,
                                                          const int* __restrict__ seg_start,
                                                          const int* __restrict__ seg_end,
                                                          const float* __restrict__ part, EmbTables tb) {
    const int lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long i = tile * EMB_RUN + lane;
    const int col = blockIdx.y * 256 + lane * 4;
    int k = tb.key_end;
    if (i < n) k = skey[i];
    bool first = false;
    if (k >= 0 && k < tb.key_end) first = seg_start[k] == i && seg_end[k] - i > EMB_RUN;
    const uint64_t m = __ballot(first);
    if (m == 0) return;
    const int L = __ffsll((unsigned long long)m) - 1;
    const int kk = __shfl(k, L);
    const int s = (int)(tile * EMB_RUN) + L, e = seg_end[kk];
    if (col >= hidden) return;
    const int nrun = (e - s + EMB_RUN - 1) / EMB_RUN;
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nrun; j += EMB_BATCH) {
        f32x4 v[EMB_BATCH];
#pragma unroll
        for (int u = 0; u < EMB_BATCH; ++u) {
            const int p = s + (j + u) * EMB_RUN;
            const long slot = 2L * (p / EMB_RUN) + (e - p >= EMB_RUN ? 1 : 0);
            v[u] = j + u < nrun ? *reinterpret_cast<const f32x4*>(part + slot * hidden + col) : tot;
        }
#pragma unroll
        for (int u = 0; u < EMB_BATCH; ++u)
            if (j + u < nrun) tot = (j + u == 0) ? v[u] : tot + v[u];
    }
    row_add(table_row(tb, kk, hidden), col, tot);
}

inline size_t up16(size_t b) { return (b + 15) / 16 * 16; }

// 0 = done, -1 = the workspace cannot hold this call (the caller runs the atomic kernels), > 0 = launch error
int text_embed_bwd_ordered(hipStream_t st, int batch, int n_tok, int hidden, int vocab, int n_types, int n_tasks,
                           const int64_t* ids, const int64_t* seg, const int64_t* task_ids, const float* dx,
                           float* dword, float* dpos, float* dtype, float* dtask, void* ws, size_t ws_bytes,
                           bool skip_pos0, bool skip_type0) {
    const int n_out = n_tok + (task_ids != nullptr ? 1 : 0);
    const long rows = (long)batch * n_out;
    const long n = 3 * rows;
    const long key_end = (long)vocab + n_tok + n_types + (task_ids != nullptr ? n_tasks : 0);
    if (ws == nullptr || n >= (1L << 30) || key_end >= EMB_MAX_KEYS) return -1;
    const long nblk = (n + SORT_TILE - 1) / SORT_TILE;
    const long ntiles = (n + EMB_RUN - 1) / EMB_RUN;
    const size_t b_arr = up16((size_t)n * 4), b_hist = up16((size_t)SORT_BUCKETS * nblk * 4),
                 b_keys = up16((size_t)key_end * 4), b_part = (size_t)2 * ntiles * hidden * 4;
    if (4 * b_arr + b_hist + 2 * b_keys + b_part > ws_bytes) return -1;
    char* w = static_cast<char*>(ws);
    int* keys_a = reinterpret_cast<int*>(w);
    int* vals_a = reinterpret_cast<int*>(w + b_arr);
    int* keys_b = reinterpret_cast<int*>(w + 2 * b_arr);
    int* vals_b = reinterpret_cast<int*>(w + 3 * b_arr);
    int* hist = reinterpret_cast<int*>(w + 4 * b_arr);
    int* seg_start = reinterpret_cast<int*>(w + 4 * b_arr + b_hist);
    int* seg_end = reinterpret_cast<int*>(w + 4 * b_arr + b_hist + b_keys);
    float* part = reinterpret_cast<float*>(w + 4 * b_arr + b_hist + 2 * b_keys);

    EmbKeys k;
    k.n_tok = n_tok;
    k.n_out = n_out;
    k.rows = (int)rows;
    k.vocab = vocab;
    k.n_types = n_types;
    k.n_tasks = task_ids != nullptr ? n_tasks : 0;
    k.key_pos = vocab;
    k.key_type = vocab + n_tok;
    k.key_task = vocab + n_tok + n_types;
    k.key_end = (int)key_end;
    k.ids = ids;
    k.seg = seg;
    k.task_ids = task_ids;
    k.skip_pos0 = skip_pos0;
    k.skip_type0 = skip_type0;
    EmbTables tb{dword, dpos, dtype, dtask, k.key_pos, k.key_type, k.key_task, k.key_end};

    const dim3 sb(256), sg((unsigned)nblk);
    const int nh = (int)(SORT_BUCKETS * nblk);
    hipLaunchKernelGGL((emb_sort_hist_kernel<true>), sg, sb, 0, st, k, (int)n, (const int*)nullptr, 0, hist, (int)nblk);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_sort_scan_kernel, dim3(1), dim3(1024), 0, st, hist, nh);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL((emb_sort_scatter_kernel<true>), sg, sb, 0, st, k, (int)n, (const int*)nullptr,
                       (const int*)nullptr, 0, (const int*)hist, (int)nblk, keys_a, vals_a);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL((emb_sort_hist_kernel<false>), sg, sb, 0, st, k, (int)n, (const int*)keys_a, SORT_BITS, hist,
                       (int)nblk);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_sort_scan_kernel, dim3(1), dim3(1024), 0, st, hist, nh);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL((emb_sort_scatter_kernel<false>), sg, sb, 0, st, k, (int)n, (const int*)keys_a,
                       (const int*)vals_a, SORT_BITS, (const int*)hist, (int)nblk, keys_b, vals_b);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (int)n, k.key_end,
                       (const int*)keys_b, seg_start, seg_end);
    VB_LAUNCH_CHECK();
    const dim3 rg((unsigned)((ntiles + 3) / 4), (unsigned)((hidden + 255) / 256));
    hipLaunchKernelGGL(emb_run_kernel, rg, dim3(256), 0, st, (int)n, hidden, (const int*)keys_b, (const int*)vals_b,
                       (const int*)seg_start, (const int*)seg_end, dx, part, tb);
    VB_LAUNCH_CHECK();
    hipLaunchKernelGGL(emb_combine_kernel, rg, dim3(256), 0, st, (int)n, hidden, (const int*)keys_b,
                       (const int*)seg_start, (const int*)seg_end, (const float*)part, tb);
    VB_LAUNCH_CHECK();
    return 0;
}

}  // namespace

namespace vbemb {

int text_embed_bwd_det(hipStream_t st, int batch, int n_tok, int hidden, int vocab, int n_types, int n_tasks,
                       const int64_t* ids, const int64_t* seg, const int64_t* task_ids, const float* dx, float* dword,
                       float* dpos, float* dtype, float* dtask, bool skip_pos0, bool skip_type0) {
    if (!vbdet::det_on()) return -1;
    size_t slice_bytes = 0;
    float* slice = vbdet::det_slice(st, &slice_bytes);
    const int r = slice != nullptr ? text_embed_bwd_ordered(st, batch, n_tok, hidden, vocab, n_types, n_tasks, ids, seg,
                                                            task_ids, dx, dword, dpos, dtype, dtask, slice, slice_bytes,
                                                            skip_pos0, skip_type0)
                                   : -1;
    if (r < 0) vbdet::det_fallback();
    return r;
}

}  // namespace vbemb
