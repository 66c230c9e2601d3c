// Host driver of tests/test_gemm_plan.py: runs every planner of csrc/gemm_plan.h over a fixed grid of launches and prints
// one line per launch. Compiled with the host C++ compiler; no GPU, no library.
//
// The operand pointers are made-up 16-byte-aligned addresses: the planners only look at their alignment, nothing here
// dereferences them. plan_v2 keeps a per-thread cache keyed by (layout, M, N, K, cseg, splits, tile code); its plan is a
// function of exactly those values, and every other planner is called afresh, so one process serves all settings.
#include <stdio.h>

#include <initializer_list>

#include "gemm_plan.h"

using namespace vbgemm;

namespace {

float* fake(uintptr_t a) { return reinterpret_cast<float*>(a); }

const char* EPI_NAME[] = {"generic", "store", "gelu", "res", "pre_gelu", "accum", "atomic", "res_drop", "dgelu", "mul"};

struct Case {
    const char* family;   // g = grid, d = MLM decoder, q = stacked q | k | v, w = wgrad fill threshold, e = epilogues, f = forced
    int layout;        // 0 = NT forward, 1 = NN dgrad, 2 = TN wgrad
    int M, N, K;       // GemmP M, N, K of that layout
    int nseg;          // stacked segments (q | k | v)
    int epi;
    int splits;        // 1, or -1 = let the planner split K
    long lda;          // 0 = the natural leading dimension
};

GemmP make(const Case& c) {
    GemmP p{};
    p.M = c.M; p.N = c.N; p.K = c.K;
    p.A = fake(0x100000);
    p.lda = c.lda ? c.lda : (c.layout == 2 ? c.M : c.K);
    for (int s = 0; s < c.nseg; ++s) p.B[s] = fake(0x200000 + 0x10000 * s);
    p.C[0] = fake(0x300000);
    p.ldc = c.N;
    p.cseg = (c.M + 127) / 128 * 128;
    if (c.layout == 0) {          // vb_linear_fwd: weight segments stacked along N
        p.ldb = c.K; p.bseg = c.N / c.nseg;
        for (int s = 0; s < c.nseg; ++s) p.bias[s] = fake(0x400000 + 0x1000 * s);
    } else if (c.layout == 1) {   // vb_linear_bwd_input: weight segments stacked along the contraction
        p.ldb = c.N; p.bseg = c.K / c.nseg;
    } else {                      // vb_linear_bwd_weight: dW segments stacked along M, the contraction runs over the rows
        p.ldb = c.N; p.bseg = c.K;
        p.cseg = c.nseg == 1 ? (c.M + 127) / 128 * 128 : c.M / c.nseg;
        for (int s = 0; s < c.nseg; ++s) {
            p.C[s] = fake(0x300000 + 0x10000 * s);
            p.colsum[s] = fake(0x500000 + 0x1000 * s);
        }
        p.accumulate = 1;
    }
    if (c.epi == EPI_RES || c.epi == EPI_RES_DROP) { p.R = fake(0x600000); p.ldr = c.N; }
    if (c.epi == EPI_DGELU) { p.D = fake(0x700000); p.ldd = c.N; }
    if (c.epi == EPI_MUL) { p.mul = fake(0x800000); p.ldmul = c.N; }
    if (c.epi == EPI_PRE_GELU) { p.P = fake(0x900000); p.ldp = c.N; }
    if (c.epi == EPI_ACCUM) p.accumulate = 1;
    p.epi = c.epi;
    p.ktiles_per_split = (c.K + 15) / 16;
    return p;
}

bool run_v2(const PlanKnobs& kn, const Case& c, const GemmP& p, V2Plan& pl) {
    if (c.layout == 0) return plan_v2<true, true>(kn, p, true, c.splits, pl);
    if (c.layout == 1) return plan_v2<true, false>(kn, p, true, c.splits, pl);
    return plan_v2<false, false>(kn, p, true, c.splits, pl);
}

// plan_v4w under `mode`: its answer and the fields it writes
void format_v4w(char (&out)[96], PlanKnobs kn, int mode, const GemmP& p0) {
    GemmP p = p0;
    kn.v4_mode = mode;
    const int c = plan_v4w(kn, p);
    snprintf(out, sizeof out, "%d,%d,%d,%d,%d,%s", c, p.tiles_n, p.n_small, p.n_big, p.ktiles_per_split, EPI_NAME[p.epi]);
}

// One line per case, "<id>\t<result>". id = family, layout, M x N x K of the GemmP, then only what differs from the
// layout's usual launch: epilogue (store; atomic for TN), splits (1; -1 for TN), segments, leading dimension of A,
// setting. result = space-separated fields, see tests/test_gemm_plan.py.
void emit(const char* setting, const PlanKnobs& kn, const Case& c) {
    const GemmP p = make(c);
    const bool tn = c.layout == 2;
    printf("%s %s %dx%dx%d", c.family, c.layout == 0 ? "NT" : c.layout == 1 ? "NN" : "TN", c.M, c.N, c.K);
    if (c.epi != (tn ? EPI_ATOMIC : EPI_STORE)) printf(" %s", EPI_NAME[c.epi]);
    if (c.splits != (tn ? -1 : 1)) printf(" splits=%d", c.splits);
    if (c.nseg != 1) printf(" nseg=%d", c.nseg);
    if (c.lda) printf(" lda=%ld", c.lda);
    if (setting[0]) printf(" %s", setting);
    V2Plan pl{};
    const bool ok = run_v2(kn, c, p, pl);
    if (ok) {
        printf("\t%d,%d,%d,%d,%d,%d,%d,%d,%a", pl.tm1, pl.tm2, pl.tn, pl.big_rows, pl.small_rows, pl.tiles_n, pl.splits,
               pl.kt_per_split, pl.cost);
        if (!tn && c.splits == 1) {   // where launch_gemm asks plan_v4: modes 0, 1, 2, then mode 1 with the small-M menu
            PlanKnobs k = kn;
            printf(" v4:");
            for (int mode = 0; mode <= 2; ++mode) {
                k.v4_mode = mode;
                printf("%d,", plan_v4(k, p, c.layout == 0, pl.cost));
            }
            k.v4_mode = 1;
            k.v4_smallm = true;
            printf("%d", plan_v4(k, p, c.layout == 0, pl.cost));
        }
        if (tn && c.splits < 0) {    // where launch_gemm asks plan_v4w (mode 0 answers -1 before it looks at the launch)
            char w1[96], w2[96];
            format_v4w(w1, kn, 1, p);
            format_v4w(w2, kn, 2, p);
            printf(" w1:%s w2:%s", w1, strcmp(w1, w2) ? w2 : "=");   // "=": mode 2 answers as mode 1
        }
    } else {
        printf("\t-");
    }
    GemmP q = p, r = p;
    plan_tiles(kn, q, 1, false);
    plan_tiles(kn, r, 1, true);
    printf(" t:%d,%d/%d,%d", q.n_big, q.n_small, r.n_big, r.n_small);
    if (tn) printf(" ws:%d", plan_wgrad_splits(kn, ((p.M + 127) / 128) * ((p.N + 127) / 128), (p.K + 15) / 16));
    if (c.layout == 1) printf(" ds:%d", plan_planes_dgrad_splits(p.M, p.N, p.K));
    printf("\n");
}

const int ROWS[] = {1628, 2304, 2368, 9216, 9472, 18432};
const int FEAT[] = {768, 1024, 2048, 2304, 3072, 4096};

template <class F>
void for_each_case(F f) {
    // the model's linears: every row count x out-features x in-features, in the three layouts
    for (int m : ROWS)
        for (int n : FEAT)
            for (int k : FEAT) {
                f(Case{"g", 0, m, n, k, 1, EPI_STORE, 1, 0});     // C[m, n] = A[m, k] W[n, k]^T
                f(Case{"g", 1, m, n, k, 1, EPI_STORE, 1, 0});     // dX[m, n] = dY[m, k] W[k, n]
                f(Case{"g", 2, n, k, m, 1, EPI_ATOMIC, -1, 0});   // dW[n, k] = dY[m, n]^T X[m, k]
            }
    // MLM decoder (30522 out-features): dgrad over the whole contraction and over its 16-aligned bulk, unsplit and
    // split-K; wgrad of the 30522 decoder rows (leading dimension 30524: room for the last float4)
    for (int kk : {30522, 30512}) {
        f(Case{"d", 1, 1628, 768, kk, 1, EPI_STORE, 1, 30522});
        f(Case{"d", 1, 1628, 768, kk, 1, EPI_ACCUM, -1, 30522});
        f(Case{"d", 1, 1628, 1024, kk, 1, EPI_ACCUM, -1, 30522});
    }
    for (int rows : {1628, 1616, 2304})
        for (int in : {768, 1024}) f(Case{"d", 2, 30522, in, rows, 1, EPI_ATOMIC, -1, 30524});
    f(Case{"d", 2, 30522, 768, 1616, 1, EPI_ATOMIC, -1, 30522});   // no room for the last float4
    f(Case{"d", 0, 1628, 30522, 768, 1, EPI_STORE, 1, 0});
    // stacked q | k | v: three segments of 768 and of 1024
    for (int seg : {768, 1024})
        for (int m : ROWS) {
            f(Case{"q", 0, m, 3 * seg, seg, 3, EPI_STORE, 1, 0});
            f(Case{"q", 1, m, seg, 3 * seg, 3, EPI_STORE, 1, 0});
            f(Case{"q", 2, 3 * seg, seg, m, 3, EPI_ATOMIC, -1, 0});
        }
    // weight gradients whose tile count puts the round-1 split rule on either side of its 93 % fill threshold
    // (94 ... 105 and 185 ... 190 tiles: there a lower r fills better than r = 4)
    for (int n : {1664, 1792, 2432, 3968})
        for (int m : {640, 768, 1024}) f(Case{"w", 2, m, n, 9216, 1, EPI_ATOMIC, -1, 0});
    // every epilogue, in every layout, unsplit and (dgrad / wgrad) split-K: plan_v2's epi_ok admits some of them
    for (int layout = 0; layout < 3; ++layout)
        for (int epi = EPI_GENERIC; epi <= EPI_MUL; ++epi)
            for (int splits : {1, -1}) {
                if (layout == 0 && splits < 0) continue;
                f(layout == 2 ? Case{"e", 2, 3072, 768, 9216, 1, epi, splits, 0}
                              : Case{"e", layout, 9216, 3072, 768, 1, epi, splits, 0});
            }
}

}  // namespace

int main() {
    printf("sizeof(GemmP)\t%zu\n", sizeof(GemmP));
    const PlanKnobs defaults;
    for_each_case([&](const Case& c) { emit("", defaults, c); });

    // forced settings on two launches per layout
    const Case few[] = {
        {"f", 0, 9216, 768, 768, 1, EPI_STORE, 1, 0},   {"f", 0, 2368, 1024, 2048, 1, EPI_STORE, 1, 0},
        {"f", 1, 9472, 1024, 1024, 1, EPI_STORE, 1, 0}, {"f", 1, 2304, 768, 2304, 3, EPI_STORE, 1, 0},
        {"f", 2, 3072, 768, 9216, 1, EPI_ATOMIC, -1, 0}, {"f", 2, 2304, 768, 2304, 3, EPI_ATOMIC, -1, 0},
    };
    char name[64];
    auto sweep = [&](const PlanKnobs& kn, int layouts) {   // layouts: bit 0 = NT and NN, bit 1 = TN
        for (const Case& c : few)
            if (layouts & (c.layout == 2 ? 2 : 1)) emit(name, kn, c);
    };
    for (int code : {22, 33, 34, 43, 44, 434, 433, 324, 323, -1}) {
        PlanKnobs kn;
        kn.tile_code = code;
        snprintf(name, sizeof name, "tile_code=%d", code);
        sweep(kn, 3);
    }
    for (int cfg : {6304, 6303, 6204, 6104, 6103, 4202, 4104, 4544, 4543}) {
        PlanKnobs kn;
        kn.v4_force_cfg = cfg;
        snprintf(name, sizeof name, "v4_force_cfg=%d", cfg);
        sweep(kn, 1);
    }
    for (int tn : {3, 4}) {
        PlanKnobs kn;
        kn.v4_tn = tn;
        snprintf(name, sizeof name, "v4_tn=%d", tn);
        sweep(kn, 1);
    }
    {
        PlanKnobs kn;
        kn.v4_menu = false;
        snprintf(name, sizeof name, "v4_menu=0");
        sweep(kn, 1);
        kn = PlanKnobs();
        kn.v4_margin = 0.5;
        snprintf(name, sizeof name, "v4_margin=0.5");
        sweep(kn, 1);
        kn = PlanKnobs();
        kn.hybrid = 0;
        snprintf(name, sizeof name, "hybrid=0");
        sweep(kn, 3);
    }
    for (int rmax : {2, 3}) {
        PlanKnobs kn;
        kn.wgrad_rmax = rmax;
        snprintf(name, sizeof name, "wgrad_rmax=%d", rmax);
        sweep(kn, 2);
    }
    return 0;
}
