// Launch planning of the fp32 GEMM family as HOST-ONLY code: the launch parameters (GemmP), every planner that
// decides which kernel and which tile / split shape a launch gets, and the settings they read (PlanKnobs). No HIP
// header and no device state: the planners are pure arithmetic on the problem shape, pointer alignment and the knobs,
// so tests/test_gemm_plan.py compiles them with the host compiler and pins their decisions
// (tests/golden/gemm_plans.json). gemm.hip owns the one PlanKnobs instance and fills it from the environment.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/vilbert_hip.h"

static inline bool vb_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// Integer / floating-point tuning variable NAME of the environment, or dflt when it is not set (api.hip).
int vb_env_int(const char* name, int dflt);
double vb_env_float(const char* name, double dflt);

namespace vbgemm {

constexpr int V2_BK = 16;   // K step of the second-generation and persistent kernels (gemm_v2.h)

// EPI_DGELU: c = gelu(v), D = gelu'(v) (the activation derivative saved for backward); EPI_MUL: c = v * mul
// (the saved derivative applied to the incoming gradient in the dgrad epilogue)
enum { EPI_GENERIC = 0, EPI_STORE, EPI_GELU, EPI_RES, EPI_PRE_GELU, EPI_ACCUM, EPI_ATOMIC, EPI_RES_DROP, EPI_DGELU,
       EPI_MUL };

struct GemmP {
    int M, N, K;
    const float* A; long lda;
    const float* B[VB_MAX_SEGMENTS]; long ldb; int bseg;   // B row segments (stacked weights)
    const float* bias[VB_MAX_SEGMENTS];
    float* C[VB_MAX_SEGMENTS]; long ldc; int cseg;          // C row segments (wgrad of stacked weights)
    float* colsum[VB_MAX_SEGMENTS];  // row-contiguous A only: colsum[i] += sum_k A[i][k] (bias gradient)
    const float* R; long ldr;
    float* P; long ldp;
    float* D; long ldd;          // activation derivative act'(pre-activation) (may be null)
    const float* mul; long ldmul;  // elementwise multiplier of the result (may be null)
    int act;
    int accumulate;       // C += result
    int tiles_n;          // big-tile grid columns
    int n_big, n_small;   // blocks [0, n_big): big tiles; [n_big, n_big + n_small): small tiles
    int m_split;          // second-generation kernel: rows [0, m_split) are cut into the taller tiles
    int ktiles_per_split; // split-K (gridDim.y > 1): atomicAdd into C
    int epi;              // EPI_* fast path of interior tiles
    int flags;            // tuning knobs (VB_GEMM_FLAGS): 1 = raise wave priority around the MFMA block
    float drop_p, drop_scale;  // dropout on the activated value, before the residual (0 = off)
    uint64_t seed;
    const uint64_t* epoch;     // device step counter mixed into the seed (vb_set_seed_epoch), may be null
    unsigned long long* dbg;   // lab only (vblab_gemm_cycles): block 0 stores its shader-clock span here
    // deterministic split-K (vb_set_deterministic): split s stores its partial product to det_ws + s * det_stride as a
    // plain [M, N] matrix (and its bias-gradient partial to det_cs + s * M) instead of adding into C with atomics; a
    // second kernel sums the partials in split order (splitk_reduce_kernel)
    float* det_ws; float* det_cs; long det_stride;
    int det_cs_parts;          // bias-gradient partials per (split, row): 1 (the plane kernels add their two k halves first)
};
// passed BY VALUE to every GEMM kernel: neither size nor field order may change
static_assert(sizeof(GemmP) == 360, "GemmP is a kernel argument: keep its layout");

// Everything the planners read from the environment or from a setter; the member initialisers are the defaults.
struct PlanKnobs {
    int gemm_mode = 0;        // VB_GEMM_MODE / vb_set_gemm_mode: bf16 operand planes (0 = exact fp32 MFMA, 3 = bf16x6, 2 = bf16x3, 1 = bf16)
    // Tile selection of the second-generation kernel: 0 = cost model, 10 TM + TN = force a menu entry (22 | 33 | 34 | 43 |
    // 44; launches it cannot serve fall back to the round-1 kernel), -1 = round-1 kernel only (VB_GEMM_V2=0 -> -1,
    // VB_GEMM_TILE=<code>, vb_set_gemm_tile)
    int tile_code = 0;
    int v4_mode = 1;          // VB_GEMM_V4 / vb_set_gemm_v4: persistent kernels 0 = never, 1 = where they fill whole rounds, 2 = wherever eligible
    int v4_force_cfg = 0;     // VB_GEMM_V4_CFG / vblab_set_gemm_v4_cfg: force one plan_v4 configuration code (0 = planner's choice)
    int v4_tn = 0;            // VB_GEMM_V4_TN: force the persistent tile width code (0 = any)
    double v4_margin = 0.98;  // VB_GEMM_V4_MARGIN: small-M menu taken when its modelled time < margin x the 4-wave time
    bool v4_menu = true;      // VB_GEMM_V4_MENU=0: the round-3 planner (288-row shapes only, >= 0.90 fill) for A/B runs
    bool v4_smallm = false;   // VB_GEMM_V4_SMALLM=1: small-M menu against the 4-wave blocks (plan_v4)
    int hybrid = 1;           // VB_GEMM_HYBRID=0: round-1 kernel without the re-cut tail (plan_tiles)
    int wgrad_rmax = 4;       // VB_WGRAD_RMAX: most blocks per CU the round-1 weight-gradient split aims for
};

// ---- second-generation kernel (gemm_v2.h): eligibility + tile / split plan --------------------------------------
// Cost model: a CU retires "16 x 16 tile K-steps" at a fixed rate once its matrix pipes are saturated, the blocks of
// a launch are dealt round-robin, so the launch takes ceil(blocks / 256) blocks of TM TN (K steps + overhead) tile
// steps on the busiest CU; eff = measured relative main-loop efficiency of the tile shape (tools/gemm_lab).
struct V2Plan { int tm1, tm2, tn, big_rows, small_rows, tiles_n, splits, kt_per_split; double cost; };

inline bool aligned_ld(const void* ptr, long ld) { return ptr == nullptr || (vb_aligned16(ptr) && ld % 4 == 0); }

// Modelled duration (arbitrary unit: one 16 x 16 tile K step on a saturated CU) of a launch of n1 tiles of area a1 (in
// 16 x 16 units) followed by n2 tiles of area a2, every block running `steps` K steps, `occ` blocks resident per CU.
// Blocks are dealt to the 256 CUs round-robin; a CU's matrix pipes are shared by its resident blocks and lose
// efficiency when fewer than 3 blocks cover each other's barriers / prologues / epilogues (occ_eff, measured).
inline double v2_launch_cost(long n1, int a1, long n2, int a2, double steps, int occ) {
    static const double occ_eff[5] = {1.0, 0.70, 0.90, 0.97, 1.0};
    double worst = 0.0;
    const long q1 = n1 / 256, r1 = n1 % 256, q2 = n2 / 256, r2 = n2 % 256;
    // the CU classes of a round-robin deal: (extra big tile?, extra small tile?)
    for (int cls = 0; cls < 4; ++cls) {
        const bool x1 = cls & 1, x2 = cls & 2;
        // CUs [0, r1) hold an extra big tile; the small tiles continue the deal at CU r1: CUs [r1, r1 + r2) mod 256
        long cnt;   // number of CUs in this class
        const long lo2 = r1, hi2 = r1 + r2;   // extra-small range, may wrap
        auto in2 = [&](long c) { return hi2 <= 256 ? (c >= lo2 && c < hi2) : (c >= lo2 || c < hi2 - 256); };
        cnt = 0;
        // count analytically would be fiddly; 256 iterations only when the class is otherwise plausible
        for (long c = 0; c < 256; ++c) cnt += ((c < r1) == x1) && (in2(c) == x2);
        if (cnt == 0) continue;
        const long b1 = q1 + (x1 ? 1 : 0), b2 = q2 + (x2 ? 1 : 0);
        long left1 = b1, left2 = b2;
        double t = 0.0;
        while (left1 + left2 > 0) {   // resident batches of up to occ blocks (big tiles first)
            const long take = left1 + left2 < occ ? left1 + left2 : occ;
            const long t1 = left1 < take ? left1 : take, t2 = take - t1;
            t += (double)(t1 * a1 + t2 * a2) * steps / occ_eff[take];
            left1 -= t1;
            left2 -= t2;
        }
        if (t > worst) worst = t;
    }
    return worst;
}

template <bool A_KC, bool B_KC>
bool plan_v2(const PlanKnobs& kn, const GemmP& p, bool vec, int splits, V2Plan& best) {
    const int code = kn.tile_code;
    const bool enabled = code >= 0;
    // forced tile: 10 TM + TN (single height) or 100 TM1 + 10 TM2 + TN (mixed heights)
    const int forced_tm1 = code >= 100 ? code / 100 : code / 10, forced_tm2 = code >= 100 ? (code / 10) % 10 : code / 10;
    const int forced_tn = code % 10;
    if (!enabled || !vec || p.K % V2_BK != 0 || p.N % 4 != 0) return false;
    if (!A_KC && p.M % 4 != 0 && p.lda < (p.M + 3) / 4 * 4) return false;
    if (!B_KC && p.bseg % V2_BK != 0) return false;   // a K tile must not straddle two stacked weight segments
    for (int s = 0; s < VB_MAX_SEGMENTS; ++s)
        if (!aligned_ld(p.C[s], p.ldc) || !aligned_ld(p.bias[s], 4)) return false;
    if (!aligned_ld(p.R, p.ldr) || !aligned_ld(p.D, p.ldd) || !aligned_ld(p.mul, p.ldmul)) return false;
    if (B_KC && p.bseg % 4 != 0) return false;
    constexpr bool FWD = A_KC && B_KC, DGRAD = A_KC && !B_KC;
    const int e = p.epi;
    const bool epi_ok = e == EPI_STORE || (FWD && (e == EPI_GELU || e == EPI_DGELU || e == EPI_RES_DROP)) ||
                        ((FWD || DGRAD) && e == EPI_RES) || (DGRAD && (e == EPI_MUL || e == EPI_ACCUM)) ||
                        (!A_KC && (e == EPI_ATOMIC || e == EPI_ACCUM || splits != 1)) ||
                        (DGRAD && splits < 0 && e == EPI_ACCUM);   // split-K dgrad of a small output (vb_linear_bwd_input)
    if (!epi_ok) return false;
    const bool multi_seg = p.C[1] != nullptr;
    // plans are cached per problem shape (a training step launches the same ~30 shapes thousands of times)
    struct Key { int layout, M, N, K, cseg, splits, code; };
    struct Entry { Key k; bool ok; V2Plan pl; };
    static thread_local Entry cache[64];
    static thread_local int cache_n = 0;
    const Key key{(A_KC ? 2 : 0) + (B_KC ? 1 : 0), p.M, p.N, p.K, multi_seg ? p.cseg : 0, splits, code};
    for (int i = 0; i < cache_n; ++i)
        if (!memcmp(&cache[i].k, &key, sizeof(Key))) { best = cache[i].pl; return cache[i].ok; }

    // {tm1, tm2, tn}: single-height tiles and the mixed-height pairs compiled in gemm_v2.hip
    static const int menu[9][3] = {{4, 4, 4}, {3, 3, 4}, {4, 4, 3}, {3, 3, 3}, {2, 2, 2}, {4, 3, 4}, {4, 3, 3}, {3, 2, 4}, {3, 2, 3}};
    // relative main-loop efficiency of a tile shape (tools/gemm_lab, round 2): bigger tiles move fewer bytes per FLOP
    auto eff = [](int tm, int tn) { return tm * tn >= 16 ? 1.0 : tm * tn >= 12 ? 0.98 : tm * tn >= 9 ? 0.93 : 0.80; };
    const int kt_total = p.K / V2_BK;
    double best_cost = 1e300;
    for (int c = 0; c < 9; ++c) {
        const int tm1 = menu[c][0], tm2 = menu[c][1], tn = menu[c][2];
        if (code > 0 && (tm1 != forced_tm1 || tm2 != forced_tm2 || tn != forced_tn)) continue;
        if (tm1 != tm2 && splits != 1) continue;   // mixed heights: forward / dgrad only (wgrad tiles a weight matrix)
        if (multi_seg && (tm1 != tm2 || p.cseg % (32 * tm1) != 0)) continue;   // tiles must not straddle two C row segments
        const int bm1 = 32 * tm1, bm2 = 32 * tm2;
        const int tiles_n = (p.N + 32 * tn - 1) / (32 * tn);
        const int occ = (tm1 * tn <= 9 && FWD) ? 4 : 3;
        const int max_big = tm1 == tm2 ? 0 : p.M / bm1;
        for (int nb = 0; nb <= max_big; ++nb) {
            // nb row tiles of the taller kind (mixed launches only), the rest of the rows in bm2-row tiles
            const int rest = p.M - nb * bm1;
            const int ns = tm1 == tm2 ? (p.M + bm2 - 1) / bm2 : (rest + bm2 - 1) / bm2;
            if (tm1 != tm2 && (nb == 0 || ns == 0)) continue;
            const long n1 = (long)nb * tiles_n, n2 = (long)ns * tiles_n;
            const int smax = splits < 0 ? (kt_total / 4 > 0 ? (kt_total / 4 < 96 ? kt_total / 4 : 96) : 1) : 1;
            for (int sp = 1; sp <= smax; ++sp) {
                const int per = (kt_total + sp - 1) / sp;
                if ((kt_total + per - 1) / per != sp) continue;
                const double steps = per + (sp > 1 ? 3.5 : 2.0);
                const double cost = v2_launch_cost(n1 * sp, tm1 * tn, n2 * sp, tm2 * tn, steps, occ) / eff(tm2, tn);
                if (cost < best_cost - 1e-9) {
                    best_cost = cost;
                    best = {tm1, tm2, tn, nb, ns, tiles_n, sp, per, cost};
                }
            }
        }
    }
    const bool ok = best_cost < 1e299;
    if (cache_n < 64) cache[cache_n++] = Entry{key, ok, best};
    return ok;
}

// Persistent one-block-per-CU kernel (gemm_v4.h), called after plan_v2 accepted the launch (alignment, epilogue).
// Mode (PlanKnobs::v4_mode): 0 = never, 1 = wherever its tiles fill whole rounds of the 256 CUs (default), 2 = every
// eligible launch (tests, lab).
// Measured in one process on the product library (tools/gemm_lab_prod LAB_V4_AB=1, profiles/r03_gemm_lab_v4_ab*.txt):
// +2 ... +13 % on every forward / dgrad shape of the model at M = 9216 and 18432 (137-147 TF against 120-136 for the
// 4-wave blocks on the same box), bert_large shapes included.
//
// -> configuration code WM * 1000 + TM * 100 + TM2 * 10 + TN of the persistent kernel (gemm_v4.h, dispatch_v4 in
// gemm_v2.hip), 0 = not used. Round 4: a tile menu instead of the two 288-row shapes -
//   * the round-3 shapes 288 x 128 / 288 x 96 (12 MFMA waves);
//   * MIXED 320 | 256-row tiles on 8 MFMA waves when M = 320 a + 256 (32 - a): the 37-region image stream at batch 256
//     (M = 9472 = 20 x 320 + 12 x 256) becomes exactly 32 row tiles x N / 128 column tiles - one tile per CU and round;
//   * small-M shapes (per-GPU batch 64: M = 2304 / 2368 rows - 64 tiles of 288 rows would leave 192 CUs idle): 192 x 128,
//     96 x 128, 96 x 96 (12 waves), 128 x 64, 64 x 128 (8 waves).
// Choice by a TIME model fitted to in-process A/B runs of every configuration on the model's shapes
// (tools/lab_v4_menu.sh, profiles/r04_gemm_lab_v4_menu_*.txt): a persistent launch costs
//     9.4 us  +  rounds x K steps x (ideal matrix-pipe time of one tile K step) / 0.94  +  (rounds - 1) x 12 us
// (launch + prologue + epilogue are ~9.4 us whatever the tile; every configuration's K step runs at ~0.94 of the pipe;
// an output-tile boundary inside a launch is a store burst), with the mixed launch timed by its 320-row
// tiles; the 4-wave alternative costs 0.93 x (plan_v2's modelled cost, in 32 x 32-tile K steps of 53.4 ns). The persistent
// kernel is taken when its modelled time is lower (mode 1), always when eligible (mode 2).
// PlanKnobs::v4_force_cfg forces one configuration wherever the shape allows it (laboratory, tests).
struct V4Opt { int wm, tm, tn; };
inline int plan_v4(const PlanKnobs& kn, const GemmP& p, bool b_kc, double v2_cost) {
    const int mode = kn.v4_mode;
    if (mode == 0) return 0;
    if (p.K % 32 != 0 || p.C[1] != nullptr || p.epi == EPI_ATOMIC || p.epi == EPI_GENERIC || p.epi == EPI_PRE_GELU) return 0;
    const int force_tn = kn.v4_tn;
    const int force_cfg = kn.v4_force_cfg;
    const double margin = kn.v4_margin;
    auto cols_ok = [&](int tn) {
        if (p.N % (32 * tn) != 0) return false;
        return !(b_kc && p.B[1] != nullptr && p.bseg % (32 * tn) != 0);   // a tile must not straddle two stacked weights
    };
    constexpr double CU_FLOPS = 157.3e12 / 256.0, T_FIXED = 9.4e-6, T_BOUNDARY = 12e-6, STEP_EFF = 0.94;
    const double nk = p.K / 16;
    auto model = [&](int bm, int bn, long tiles) {
        const double rounds = (double)((tiles + 255) / 256);
        return T_FIXED + rounds * nk * (2.0 * bm * bn * 16.0 / CU_FLOPS) / STEP_EFF + (rounds - 1.0) * T_BOUNDARY;
    };
    static const V4Opt menu[] = {{6, 3, 4}, {6, 3, 3}, {6, 2, 4}, {6, 1, 4}, {6, 1, 3}, {4, 2, 2}, {4, 1, 4}};
    const bool menu_on = kn.v4_menu;
    double best = 1e30;
    int best_cfg = 0;
    bool best_fills = false;
    for (const V4Opt& o : menu) {
        if (!cols_ok(o.tn) || (force_tn != 0 && force_tn != o.tn)) continue;
        const int cfg = o.wm * 1000 + o.tm * 100 + o.tn;
        if (force_cfg != 0 && force_cfg != cfg) continue;
        if (!menu_on && o.tm != 3) continue;
        const int bm = 16 * o.tm * o.wm;
        const long rows = (p.M + bm - 1) / bm, tiles = rows * (p.N / (32 * o.tn));
        const double t = model(bm, 32 * o.tn, tiles);
        if (t < best - 1e-12) {
            best = t;
            best_cfg = cfg;
            // the round-3 rule: a 288-row shape whose launched tile slots are >= 90 % useful
            best_fills = o.tm == 3 && (double)tiles / (double)((tiles + 255) / 256 * 256) * ((double)p.M / (rows * 288.0)) >= 0.90;
        }
    }
    bool best_mixed = false;
    // mixed 320 | 256-row tiles (8 MFMA waves): M = 320 a + 256 (32 - a), 0 < a < 32
    for (int tn = 4; tn >= 3 && menu_on; --tn) {
        const int cfg = 4540 + tn;
        if (!cols_ok(tn) || (p.N / (32 * tn)) % 8 != 0 || (force_cfg != 0 && force_cfg != cfg) || (force_tn != 0 && force_tn != tn)) continue;
        const int rest = p.M - 32 * 256;
        if (rest <= 0 || rest % 64 != 0 || rest / 64 >= 32) continue;
        const double t = model(320, 32 * tn, 32L * (p.N / (32 * tn)));
        if (t < best - 1e-12) { best = t; best_cfg = cfg; best_mixed = true; best_fills = false; }
    }
    if (best_cfg == 0) return 0;
    if (mode == 2 || force_cfg != 0) return best_cfg;
    // mode 1. Measured (in-process A/B on every shape of the model, profiles/r03_gemm_lab_v4_ab_*.txt,
    // r04_gemm_lab_v4_menu_*.txt): the 288-row shapes that fill the chip and the mixed launch beat the 4-wave blocks on
    // every forward / dgrad shape but one (+4 ... +14 %; 9472 x 1024 x 3 x 1024 forward: -1 %). For the small-M menu the two models are compared; plan_v2's cost is in
    // 32 x 32-tile K steps (53.4 ns on a saturated CU) and tracks the measured time (x 0.93) while a CU holds at most two
    // 4-wave blocks - beyond that (large M, where the menu has nothing to offer anyway) it is not calibrated: 4-wave.
    if (best_fills || best_mixed) return best_cfg;
    // The small-M menu wins most isolated A/Bs (profiles/r04_gemm_lab_v4_menu_M2304.txt / _M2368.txt, planner's choice against the
    // 4-wave blocks: +8 ... +20 % on 15 of 20 forward / dgrad launches, -1 ... -13 % on 5) and is a WASH inside the batch-64 training
    // step (profiles/r04_bench_b64_menu_ab.txt: 1,986 -> 2,022 samples/s eager, 1,716 -> 1,773 single-stream, 1,887 -> 1,932 as
    // one HIP graph on one box; 1,954 -> 1,866 on an earlier one): there the text / image / weight-gradient streams keep
    // several kernels in flight, the 4-wave blocks of different kernels co-reside on a CU and cover each other's bubbles,
    // while a persistent block owns its CU - so it is opt-in (VB_GEMM_V4_SMALLM=1: single-stream inference, laboratory).
    const bool small_m = kn.v4_smallm;
    if (!menu_on || !small_m) return 0;
    const long v2_tiles = (long)((p.M + 95) / 96) * ((p.N + 95) / 96);     // upper bound of plan_v2's block count
    if (v2_tiles > 3 * 256) return 0;
    const double t_v2 = 0.93 * 53.4e-9 * v2_cost;
    return best < margin * t_v2 ? best_cfg : 0;
}

// Persistent weight-gradient kernel (gemm_v4w.h): 384 x 96 tiles of dW times K splits as equal work units. Fills the
// launch fields and returns the configuration index when the shape divides (text-stream weights: 768 / 2304 / 3072
// rows, 768 / 3072 columns) and the units fill the chip, -1 otherwise.
inline int plan_v4w(const PlanKnobs& kn, GemmP& p) {
    const int mode = kn.v4_mode;
    if (mode == 0 || p.K % 32 != 0) return -1;
    // {tile rows, tile columns, relative main-loop efficiency}: 12 MFMA waves for the 384-row tiles, 8 for the 256-row ones
    static const struct { int bm, bn; double eff; } cfgs[3] = {{384, 96, 1.0}, {256, 128, 0.95}, {256, 96, 0.93}};
    const int kt = p.K / V2_BK;
    double best = 1e300;
    int best_s = 0, best_c = -1;
    for (int c = 0; c < 3; ++c) {
        const int BM = cfgs[c].bm, BN = cfgs[c].bn;
        if (p.M % BM != 0 || p.N % BN != 0 || p.cseg % BM != 0) continue;
        const long tiles = (long)(p.M / BM) * (p.N / BN);
        for (int s = 1; s <= 64; ++s) {
            if (kt % s != 0) continue;
            const int nk = kt / s;
            if (nk % 2 != 0 || nk < 8) continue;
            const long units = tiles * s, rounds = (units + 255) / 256;
            const double eff = (double)units / (double)(rounds * 256);
            // measured (tools/gemm_lab_prod LAB_V4_AB=1, profiles/r03_gemm_lab_v4w_ab.txt): +8.5 % with 144 K steps per unit
            // (W[3072, 768], W[768, 3072] at 9216 rows), -5 % with 36 (W[768, 768] needs 16 splits to fill the chip and
            // every unit ends in a 147 KB burst of stores that all 256 blocks issue at the same instant)
            if (mode != 2 && (eff < 0.85 || nk < 64)) continue;
            // ~8 K steps of epilogue per unit; cost in units of one 16 x 16 tile K step per CU
            const double cost = (double)rounds * (nk + 8.0) * (BM / 16) * (BN / 16) / cfgs[c].eff;
            if (cost < best - 1e-9) { best = cost; best_s = s; best_c = c; }
        }
    }
    if (best_c < 0) return -1;
    const int BM = cfgs[best_c].bm, BN = cfgs[best_c].bn;
    const long tiles = (long)(p.M / BM) * (p.N / BN);
    p.tiles_n = p.N / BN;
    p.n_small = (int)tiles;
    p.n_big = (int)(tiles * best_s);
    p.ktiles_per_split = kt / best_s;
    p.epi = best_s > 1 ? EPI_ATOMIC : EPI_ACCUM;
    return best_c;
}

// Round-1 kernel. Tile plan: full rounds of 256 big tiles, leftover as small tiles when that shortens the tail.
inline void plan_tiles(const PlanKnobs& kn, GemmP& p, int splits, bool planes_mode) {
    const int tiles_m = (p.M + 127) / 128;
    p.tiles_n = (p.N + 127) / 128;
    const int total = tiles_m * p.tiles_n;
    const int hybrid = kn.hybrid;
    const int left = total % 256;
    // 4 * left small tiles cost ceil(4 left / 256) quarter-rounds vs one full big round (= 4). A small tile
    // runs at ~3/4 of a big tile's MFMA efficiency in the fp32 kernel (re-cut when < 4 quarter-rounds) but
    // at ~1/2 in the bf16-planes kernel, whose per-thread split work does not shrink with the tile
    // (re-cut only when the tail fits ONE quarter-round).
    const int limit = planes_mode ? 2 : 4;
    const bool recut = hybrid && splits == 1 && left > 0 && (4 * left + 255) / 256 < limit && (p.cseg % 64) == 0;
    p.n_big = recut ? total - left : total;
    p.n_small = recut ? 4 * left : 0;
}

// Round-1 / bf16-planes weight gradient (vb_linear_bwd_weight), `tiles` 128 x 128 output tiles over kt_total K tiles.
// Split count: tiles x splits workgroups should fill r whole "one block per CU" rounds of the 256
// CUs (all co-resident, so r = blocks per CU) WITHOUT spilling into a partial extra round.
// Measured: r = 4 beats fewer, longer blocks (one block per CU leaves the matrix pipe idle during
// every barrier / epilogue); take the largest r <= 4 that fills >= 93 % of its slots.
inline int plan_wgrad_splits(const PlanKnobs& kn, int tiles, int kt_total) {
    int splits = 1;
    double best = -1.0;
    const int rmax = kn.wgrad_rmax;
    for (int r = rmax; r >= 2; --r) {
        int s = (256 * r) / tiles;
        if (s < 1) s = 1;
        if (s > kt_total / 4) s = kt_total / 4 > 0 ? kt_total / 4 : 1;  // >= 4 K tiles per block
        const int blocks = tiles * s;
        const double fill = (double)blocks / (256.0 * ((blocks + 255) / 256));
        if (fill > best + 1e-9) { best = fill; splits = s; }
        if (fill >= 0.93) break;
    }
    return splits;
}

// Split-K input gradient of a small output with a long contraction in the bf16-plane modes (vb_linear_bwd_input):
// about three blocks per CU, at least 1024 contraction elements per split, at most 32 splits.
inline int plan_planes_dgrad_splits(int M, int N, int K) {
    const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
    long sp = (768 + tiles - 1) / tiles;
    if (sp > K / 1024) sp = K / 1024;
    return (int)(sp < 1 ? 1 : (sp > 32 ? 32 : sp));
}

}  // namespace vbgemm
