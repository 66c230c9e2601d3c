// Which output tile (or work unit) a block of a PERSISTENT launch takes in which round: the one map of every persistent
// kernel of the library - the fp32 kernels of gemm_v4.h / gemm_v4w.h, the bf16 training kernels of gemm_bf16.hip and the MX
// kernel of mx8.hip. A wrong map writes an output tile twice or never, so it exists once, and the index arithmetic is
// plain C++ without a HIP header: tests/test_persistent_map.py compiles it with the host compiler and checks, for every
// tile count around whole and partial rounds, that each tile is handed out exactly once. Device code gets the same
// functions as __host__ __device__, plus the LDS-DMA wrapper of the loader waves (device only).
#pragma once

#if defined(__HIP__)
#define VB_MAP_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define VB_MAP_FN static inline
#endif

namespace vbgemm {

// tile of block `b` in round `it` of a persistent launch over `tiles` output tiles on `grid` blocks, -1 = none (the block
// is done: a block's rounds are contiguous, which is what the kernels' `while (rounds * grid < tiles && tile_of(...) >= 0)`
// loops count). Round `it` hands out the tiles [it grid, (it + 1) grid). The blocks of one XCD (b % 8) work on a
// contiguous run of them at any time - XCD x takes [x per, (x + 1) per), per = n / 8 - so that they share A / W panels in
// their L2; a round whose tile count is no multiple of 8 (only ever the last) is dealt block by block.
VB_MAP_FN int tile_of(int b, int it, int grid, int tiles) {
    const int base = it * grid;
    const int n = grid < tiles - base ? grid : tiles - base;   // tiles of this round
    if (n <= 0) return -1;
    if ((n & 7) != 0) return b < n ? base + b : -1;
    const int per = n >> 3, x = b & 7, j = b >> 3;
    return j < per ? base + x * per + j : -1;
}

// (row, column) of output tile `t` of a tiles / tiles_n x tiles_n tile grid. The 32 tiles an XCD works on at any time
// (tile_of) should share as few A / W panels as possible: where the tile grid allows it they form a 4 x 8 patch (4 A
// panels + 8 W panels per XCD and round instead of 1.3 + 24 for a 24-column grid walked row by row: measured 7.0x -> see
// profiles/r03_gemm_pmc.txt for the operand bytes fetched through the fabric per launch); other grids are walked row by
// row (N fastest).
VB_MAP_FN void tile_rc(int t, int tiles, int tiles_n, int& r, int& c) {
    const int tiles_m = tiles / tiles_n;
    if ((tiles_n & 7) == 0 && (tiles_m & 3) == 0) {
        const int patch = t >> 5, w = t & 31, pcols = tiles_n >> 3;
        r = (patch / pcols) * 4 + (w >> 3);
        c = (patch % pcols) * 8 + (w & 7);
    } else {
        r = t / tiles_n;
        c = t % tiles_n;
    }
}

// work unit of block `b` in its i-th round, for launches whose unit count is NOT made a multiple of 8 (the bf16 weight
// gradient: units = output tiles x contraction splits; grid = a multiple of 8): XCD x takes the units [x per, (x + 1) per)
// of the round, per = ceil(n / 8) - the same contraction split and neighbouring output tiles, so that the row range of
// dY / X they stream is shared in their L2. Same contract as tile_of: -1 = none, a block's rounds are contiguous.
VB_MAP_FN int unit_of(int b, int i, int grid, int units) {
    const int base = i * grid;
    const int n = grid < units - base ? grid : units - base;
    if (n <= 0) return -1;
    const int per = (n + 7) >> 3, x = b & 7, j = b >> 3;
    const int idx = x * per + j;
    return (j < per && idx < n) ? base + idx : -1;
}

#if defined(__HIP__)
// one LDS-DMA, lean form for the loaders' inner loops: LDS[lds + 16 lane] <- *(base + off[lane]). The source address is
// a wave-uniform 64-bit base (SGPR pair, advanced once per K step) plus a per-lane 32-bit byte offset that is constant
// for a whole output tile, so a K step costs the loader 3 instructions per DMA and no vector ALU work at all. (The
// first version bumped a 64-bit pointer per lane per DMA and saved / restored M0 around each one: 3,658 cycles per K step
// to issue 24 DMAs - more than the 3,456 matrix-pipe cycles of the step, measured with the lab's loader counters.)
// M0 is not preserved: nothing else in a loader wave uses it.
__device__ __forceinline__ void glds16(unsigned off, const void* base, unsigned lds) {
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(base), "s"(lds) : "memory");
}
#endif

}  // namespace vbgemm

#undef VB_MAP_FN
