// Host driver of tests/test_dropout_mask.py: evaluates csrc/rng.h - the mask function of every dropout site of the library -
// on the CPU. The header is device code without any device intrinsic: with the two qualifiers defined away it compiles
// unchanged with the host C++ compiler; no GPU, no library.
//
// stdin: raw records {uint64 seed, uint64 idx, float p, uint32 unused}; stdout: one record {uint32 vb_hash(seed, idx),
// uint32 vb_keep(seed, idx, p), uint64 vb_seed_with_epoch(seed, &idx), uint64 vb_seed_with_epoch(seed, nullptr)} each (idx
// doubles as the step counter's value).
#include <stdint.h>
#include <stdio.h>

#include <vector>

#define __device__
#define __forceinline__ inline
#include "rng.h"

struct In { uint64_t seed, idx; float p; uint32_t unused; };
struct Out { uint32_t hash, keep; uint64_t with_epoch, without_epoch; };
static_assert(sizeof(In) == 24 && sizeof(Out) == 24, "record layout");

int main() {
    std::vector<In> in(1 << 14);
    std::vector<Out> out(in.size());
    size_t n;
    while ((n = fread(in.data(), sizeof(In), in.size(), stdin)) > 0) {
        for (size_t i = 0; i < n; ++i) {
            const uint64_t counter = in[i].idx;
            out[i].hash = vb_hash(in[i].seed, in[i].idx);
            out[i].keep = vb_keep(in[i].seed, in[i].idx, in[i].p) ? 1u : 0u;
            out[i].with_epoch = vb_seed_with_epoch(in[i].seed, &counter);
            out[i].without_epoch = vb_seed_with_epoch(in[i].seed, nullptr);
        }
        if (fwrite(out.data(), sizeof(Out), n, stdout) != n) return 1;
    }
    return 0;
}
