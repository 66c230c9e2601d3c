// Host driver of tests/test_persistent_map.py: evaluates the block-to-tile map of csrc/persistent_map.h over a fixed grid and
// writes the raw results to stdout as int32. Compiled with the host C++ compiler; no GPU, no library. All checking is done
// by the test.
//   for grid in GRIDS, n in 1 .. 3 grid + 9, round in 0 .. ceil(n / grid) (one past the last), b in 0 .. grid - 1:
//       tile_of(b, round, grid, n)            ... then the same loops again for unit_of
//   for tiles_n in 1 .. 32, tiles_m in 1 .. 80, t in 0 .. tiles_m tiles_n - 1:  r, c of tile_rc
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "persistent_map.h"

using namespace vbgemm;

int main() {
    const int GRIDS[] = {8, 16, 64, 128, 160, 256, 512};
    std::vector<int32_t> out;
    for (int which = 0; which < 2; ++which)
        for (int grid : GRIDS)
            for (int n = 1; n <= 3 * grid + 9; ++n)
                for (int it = 0; it <= (n + grid - 1) / grid; ++it)
                    for (int b = 0; b < grid; ++b) out.push_back(which == 0 ? tile_of(b, it, grid, n) : unit_of(b, it, grid, n));
    for (int tiles_n = 1; tiles_n <= 32; ++tiles_n)
        for (int tiles_m = 1; tiles_m <= 80; ++tiles_m)
            for (int t = 0; t < tiles_m * tiles_n; ++t) {
                int r = -1, c = -1;
                tile_rc(t, tiles_m * tiles_n, tiles_n, r, c);
                out.push_back(r);
                out.push_back(c);
            }
    return fwrite(out.data(), sizeof(int32_t), out.size(), stdout) == out.size() ? 0 : 1;
}
