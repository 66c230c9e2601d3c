// Which rows of the flat region-target table [batch * regions, dim] a labelled region is contrasted with in the NCE
// region loss (visual_target == 2; reference vilbert.py:1532-1557): the ONE function from (seed, labelled region, draw) to
// a negative's row. Counter-based like the dropout mask (rng.h): nothing is stored between launches, a test restates every
// index on the host (tests/nce_restatement.py), and the index depends on the REGION, not on the row's position in a gather -
// the exact and the fixed-capacity gather of the labelled rows draw the same negatives.
// Plain C++ without a HIP header: tests/nce_index_driver.cpp compiles it with the host compiler; device code (nce.hip) gets
// the same functions as __host__ __device__.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define VB_NCE_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define VB_NCE_FN static inline
#endif

namespace vbnce {

// rng.h vb_hash, restated host-callable (rng.h itself stays device code for its users; tests/test_nce_index.py holds the two
// to one numpy restatement): upper 32 bits of the splitmix64 finaliser over seed + idx * golden ratio
VB_NCE_FN uint32_t hash(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + idx * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    return (uint32_t)(z >> 32);
}

// uniform 32-bit word -> [0, m), m <= 2^32 - 1 (multiply-shift: no division, no rejection loop)
VB_NCE_FN uint32_t scale(uint32_t x, uint32_t m) { return (uint32_t)(((uint64_t)x * m) >> 32); }

// Negative j (0 <= j < n_across + n_inside) of labelled region g = b * regions + r (regions: WITHOUT the global row) under
// launch seed s (after vb_seed_with_epoch). Draw k of (g, j) is hash(s, (g * n_neg + j) * 2 + k).
//   j <  n_across  "across": a region of ANOTHER sample - sample scale(h0, batch - 1), b itself remapped to batch - 1 (the
//                  reference's random_(0, B - 1) followed by row[row == i] = B - 1), region scale(h1, regions);
//   j >= n_across  "inside": another region of the SAME sample - scale(h1, regions - 1), r itself remapped to regions - 1.
// Needs batch >= 2 for an across draw and regions >= 2 for an inside draw (checked by the launcher).
VB_NCE_FN int64_t negative_row(uint64_t s, int64_t g, int32_t j, int32_t batch, int32_t regions, int32_t n_across,
                               int32_t n_inside) {
    const int64_t b = g / regions, r = g - b * regions;
    const uint64_t at = ((uint64_t)g * (uint64_t)(n_across + n_inside) + (uint64_t)j) * 2u;
    if (j < n_across) {
        int64_t rb = scale(hash(s, at), (uint32_t)(batch - 1));
        if (rb == b) rb = batch - 1;
        const int64_t rc = scale(hash(s, at + 1), (uint32_t)regions);
        return rb * regions + rc;
    }
    int64_t rc = scale(hash(s, at + 1), (uint32_t)(regions - 1));
    if (rc == r) rc = regions - 1;
    return b * regions + rc;
}

}  // namespace vbnce
