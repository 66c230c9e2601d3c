// Launch planning of the bf16 training GEMMs (gemm_bf16.hip) as HOST-ONLY code, after gemm_plan.h: which block shape and
// persistent grid a forward / input-gradient launch gets (plan_hb), how many contraction splits a weight gradient gets and
// whether it takes the deterministic workspace slice (plan_hw), and the settings both read (Bf16Knobs). No HIP header and
// no environment read: pure arithmetic on the problem shape and the knobs, so tests/test_gemm_bf16_plan.py compiles it
// with the host compiler and pins its decisions (tests/golden/gemm_bf16_plans.json) - an edit of the split rule changes
// both speed and the deterministic-workspace footprint. gemm_bf16.hip owns the one Bf16Knobs instance and fills it from
// the environment.
#pragma once
#include <stddef.h>

namespace vbgemm {

// output tile of the full-size block / contraction tile: 256 x 128 x 64 (the weight gradient tiles dW the same way: 256
// rows of n x 128 columns of k, 64 rows of m per contraction tile)
constexpr int HB_BM = 256, HB_BN = 128, HB_BK = 64;

// Everything the planners read from the environment; the member initialisers are the defaults.
struct Bf16Knobs {
    // VB_BF16_GRID: persistent blocks per launch (a multiple of 8 in 8 .. 256, default = the 256 CUs): with fewer, two
    // launches of different streams share the chip side by side instead of one after the other
    int grid_limit = 256;
    // VB_BF16_HALF: 0 = always the full-size block, 2 = always two half-size blocks per CU, 1 = see plan_hb
    int half = 1;
    // VB_BF16_WG_TK / _TE / _TD: the weight-gradient time model of plan_hw, microseconds
    float t_k = 1.0f, t_e = 0.12f, t_d = 0.04f;
};

// NT kernel (forward, input gradient): rows of an output tile (256: one full-size block per CU; 128: two half-size blocks
// per CU), output tiles, blocks per CU, blocks of the persistent launch.
// VB_BF16_HALF = 1 (default): the half-size blocks for launches of at most 128 full-size tiles (the per-GPU batch 64
// shapes: 80 tiles on 256 CUs become 160 blocks - 23.5 -> 16.6 us at 2368 x 1024 x 1024). Everywhere else the half-size
// block LOSES (profiles/r05_bf16_half_blocks.txt): a 128 x 128 tile reads a third more operand bytes per FLOP through L2 /
// LDS-DMA, and the main loop alone falls from ~1.0 PF to 0.62 - 0.74 PF - more than the overlapped epilogues win back (q|k|v
// forward 44.8 -> 67.7 us).
struct HbPlan { int bm, tiles, per_cu, grid; };
static inline HbPlan plan_hb(int M, int tiles_n, const Bf16Knobs& kn) {
    const int tiles_full = ((M + 255) / 256) * tiles_n;
    const bool use_half = kn.half == 2 || (kn.half == 1 && tiles_full <= 128);
    HbPlan pl;
    pl.bm = use_half ? 128 : 256;
    pl.per_cu = use_half ? 2 : 1;
    pl.tiles = ((M + pl.bm - 1) / pl.bm) * tiles_n;
    const int slots = kn.grid_limit * pl.per_cu;
    pl.grid = pl.tiles < slots ? pl.tiles : slots;
    return pl;
}

// TN kernel (weight gradient dW[N, K] of M rows). slice_bytes = size of the deterministic workspace slice the launch may
// use, 0 = none (the setting is off, or the stream has no slice).
// Contraction splits by a time model (measured with the laboratory flags, profiles/r05_bf16_lab_ablations.txt): a unit's
// main loop costs ~1.0 us per contraction tile (t_k), its epilogue - 128 KiB of fp32 atomics that execute at the memory
// side, ~1.7 TB/s for the whole chip - ~0.075 us per unit IN FLIGHT ANYWHERE (t_e = 0.12 in the model: in the step, where
// other streams compete for the memory side, fewer splits measured +0.7 %); rounds of 256 units. More splits shorten the
// main loop and lengthen the atomics: the first version's "fill two rounds" rule spent 30 - 50 % of a launch in atomics.
// Deterministic form: a unit's 128 KiB leave as plain 16-byte stores (t_d per unit), and the reduce pass reads every
// partial once and updates dW: (splits + 2) x 4 N K bytes at ~3.5 TB/s + its launch; only split counts whose partials fit
// the slice are candidates. The candidates are tried in rising order and a later one wins only when it is strictly
// faster.
struct HwPlan {
    int tiles, nkt;  // 256 x 128 tiles of dW, 64-row contraction tiles of M: what splits / units / grid were planned for
    int splits, kt_per_split, units, grid;
    bool use_ws;     // the units store partial tiles to the slice and the reduce kernel follows; false = fp32 atomics
    bool fallback;   // a slice was offered and not even one split fits it: counted by vb_deterministic_fallbacks
};
static inline HwPlan plan_hw(int M, int N, int K, size_t slice_bytes, const Bf16Knobs& kn) {
    const float t_k = kn.t_k, t_e = kn.t_e, t_d = kn.t_d;
    const int tiles = (N / HB_BM) * (K / HB_BN);
    const int nkt = (M + HB_BK - 1) / HB_BK;
    // A slice of 0 bytes counts as no slice: the atomics time model picks the splits, where a non-null slice of 0 bytes
    // used to fail every candidate and run unsplit. Only a registered workspace of under 16 bytes per slice yields one
    // (det_workspace.hip), no partial tile fits it either way, and the launcher counts the fallback in both cases, by
    // "deterministic and not use_ws".
    bool ws = slice_bytes != 0;
    const size_t per_split = ((size_t)tiles * 32768 + (size_t)N) * sizeof(float);
    int best = 1;
    float best_t = 1e30f;
    for (int sp = 1; sp <= nkt && sp <= 64; ++sp) {
        const int per = (nkt + sp - 1) / sp, real = (nkt + per - 1) / per;
        if (real != sp) continue;
        const long units = (long)tiles * sp;
        float t = (float)((units + 255) / 256) * (per * t_k + 2.0f);
        if (ws) {
            if ((size_t)sp * per_split > slice_bytes) continue;
            t += units * t_d + 3.0f + (float)(sp + 2) * (4.0f * N * K) / 3.5e6f;
        } else {
            t += units * t_e;
        }
        if (t < best_t) { best_t = t; best = sp; }
    }
    if (best_t >= 1e30f) ws = false;          // (not even one split fits the slice)
    HwPlan pl;
    pl.tiles = tiles;
    pl.nkt = nkt;
    pl.kt_per_split = (nkt + best - 1) / best;
    pl.splits = (nkt + pl.kt_per_split - 1) / pl.kt_per_split;
    pl.units = tiles * pl.splits;
    pl.grid = pl.units < kn.grid_limit ? (pl.units + 7) / 8 * 8 : kn.grid_limit;
    pl.use_ws = ws;
    pl.fallback = slice_bytes != 0 && !ws;
    return pl;
}

}  // namespace vbgemm
