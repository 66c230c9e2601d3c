// Host driver of tests/test_gemm_planes_host.py: the three launch decisions of csrc/gemm_plan.h that the direct tests of the
// bf16-plane kernel rely on, for the launches given on the command line. Compiled with the host C++ compiler; no GPU, no library.
//   t M N splits planes_mode cseg   -> plan_tiles n_big n_small
//   w tiles kt_total                -> plan_wgrad_splits
//   d M N K                         -> plan_planes_dgrad_splits
#include <stdio.h>
#include <stdlib.h>

#include "gemm_plan.h"

using namespace vbgemm;

int main(int argc, char** argv) {
    const PlanKnobs kn;
    for (int i = 1; i < argc;) {
        const char kind = argv[i][0];
        if (kind == 't' && i + 5 < argc) {
            GemmP p{};
            p.M = atoi(argv[i + 1]); p.N = atoi(argv[i + 2]); p.cseg = atoi(argv[i + 5]);
            plan_tiles(kn, p, atoi(argv[i + 3]), atoi(argv[i + 4]) != 0);
            printf("%d %d\n", p.n_big, p.n_small);
            i += 6;
        } else if (kind == 'w' && i + 2 < argc) {
            printf("%d\n", plan_wgrad_splits(kn, atoi(argv[i + 1]), atoi(argv[i + 2])));
            i += 3;
        } else if (kind == 'd' && i + 3 < argc) {
            printf("%d\n", plan_planes_dgrad_splits(atoi(argv[i + 1]), atoi(argv[i + 2]), atoi(argv[i + 3])));
            i += 4;
        } else {
            return 2;
        }
    }
    return 0;
}
