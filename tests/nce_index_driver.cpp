// Host driver of tests/test_nce_index.py: evaluates csrc/nce_index.h - the negative rows of the NCE region loss - on the CPU.
// The header is plain C++ for the host compiler too; the launch seed goes through rng.h's vb_seed_with_epoch as in the
// kernel (rng.h is device code without any device intrinsic: with the two qualifiers defined away it compiles unchanged).
//
// stdin: raw records {uint64 seed, uint64 epoch, int64 g, int32 batch, regions, n_across, n_inside, j, use_epoch};
// stdout: one record {int64 row, uint32 hash(seed, g) of nce_index.h, uint32 vb_hash(seed, g) of rng.h} each.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#define __device__
#define __forceinline__ inline
#include "rng.h"

#include "nce_index.h"

struct In { uint64_t seed, epoch; int64_t g; int32_t batch, regions, n_across, n_inside, j, use_epoch; };
struct Out { int64_t row; uint32_t hash_nce, hash_rng; };
static_assert(sizeof(In) == 48 && sizeof(Out) == 16, "record layout");

int main() {
    std::vector<In> in(1 << 14);
    std::vector<Out> out(in.size());
    size_t n;
    while ((n = fread(in.data(), sizeof(In), in.size(), stdin)) > 0) {
        for (size_t i = 0; i < n; ++i) {
            const In& q = in[i];
            const uint64_t s = vb_seed_with_epoch(q.seed, q.use_epoch ? &q.epoch : nullptr);
            out[i].row = vbnce::negative_row(s, q.g, q.j, q.batch, q.regions, q.n_across, q.n_inside);
            out[i].hash_nce = vbnce::hash(q.seed, (uint64_t)q.g);
            out[i].hash_rng = vb_hash(q.seed, (uint64_t)q.g);
        }
        if (fwrite(out.data(), sizeof(Out), n, stdout) != n) return 1;
    }
    return 0;
}
