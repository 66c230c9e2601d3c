// Host driver of tests/test_gemm_bf16_plan.py: runs the planners of csrc/gemm_bf16_plan.h over a fixed grid of launches and
// prints one line per launch, "<id>\t<result>". Compiled with the host C++ compiler; no GPU, no library.
//   hb <N>x<M> half=<VB_BF16_HALF> grid=<VB_BF16_GRID>          -> bm,tiles,per_cu,grid   (C[M, N]; the rows come last in both ids)
//   hw <N>x<K>x<M> nseg=<segments of N> slice=<MiB>             -> splits,kt_per_split,units,grid,<ws | atomics | fallback>
// extra arguments "hw N K M slice_bytes" (any number of such groups): only those weight-gradient launches, default knobs,
// ids "hw <N>x<K>x<M> bytes=<slice_bytes>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "gemm_bf16_plan.h"

using namespace vbgemm;

namespace {

const int ROWS[] = {1628, 2304, 2368, 9216, 9472, 18432};
const int FEAT[] = {768, 1024, 2304, 3072, 4096};

void emit_hw(const char* id_tail, int N, int K, int M, size_t slice_bytes, const Bf16Knobs& kn) {
    const HwPlan pl = plan_hw(M, N, K, slice_bytes, kn);
    printf("hw %dx%dx%d%s\t%d,%d,%d,%d,%s\n", N, K, M, id_tail, pl.splits, pl.kt_per_split, pl.units, pl.grid,
           pl.fallback ? "fallback" : pl.use_ws ? "ws" : "atomics");
}

}  // namespace

int main(int argc, char** argv) {
    const Bf16Knobs defaults;
    if (argc > 1) {
        for (int i = 1; i + 4 < argc && !strcmp(argv[i], "hw"); i += 5) {
            char tail[48];
            snprintf(tail, sizeof tail, " bytes=%s", argv[i + 4]);
            emit_hw(tail, atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3]), (size_t)strtoull(argv[i + 4], nullptr, 10), defaults);
        }
        return 0;
    }
    for (int half = 0; half <= 2; ++half)
        for (int limit : {256, 128})
            for (int m : ROWS)
                for (int n : FEAT) {
                    Bf16Knobs kn;
                    kn.half = half;
                    kn.grid_limit = limit;
                    const HbPlan pl = plan_hb(m, n / HB_BN, kn);
                    printf("hb %dx%d half=%d grid=%d\t%d,%d,%d,%d\n", n, m, half, limit, pl.bm, pl.tiles, pl.per_cu, pl.grid);
                }
    // the model's weights: seg_n x K over the feature list (every entry is a multiple of 256 and of 128), alone and as three
    // stacked segments (q | k | v), with no slice, the default-sized one and a deliberately small one
    for (int nseg : {1, 3})
        for (int seg_n : FEAT)
            for (int k : FEAT)
                for (int m : ROWS)
                    for (int mib : {0, 256, 64}) {
                        if (seg_n % HB_BM != 0 || k % HB_BN != 0) continue;
                        char tail[48];
                        snprintf(tail, sizeof tail, " nseg=%d slice=%d", nseg, mib);
                        emit_hw(tail, nseg * seg_n, k, m, (size_t)mib << 20, defaults);
                    }
    return 0;
}
