// Host driver of tests/test_row_checks_host.py: the argument checks and launch arithmetic of the row kernels
// (csrc/row_checks.h) at their boundaries. Compiled with the host C++ compiler (and its sanitizers where it has them); no GPU,
// no library. Prints "<case>\t<value>" per line; all checking is done by the test.
#include <stdint.h>
#include <stdio.h>

#include "row_checks.h"

namespace {

alignas(16) char g_buf[32];

void show(const char* name, long long v) { printf("%s\t%lld\n", name, v); }

}  // namespace

int main() {
    const int64_t big = INT64_MAX;
    show("extent_0_max", vb_extent_ok(0, big));
    show("extent_neg_max", vb_extent_ok(-1, big));
    show("extent_1_max", vb_extent_ok(1, big));
    show("extent_2_half", vb_extent_ok(2, big / 2));
    show("extent_2_half_plus_1", vb_extent_ok(2, big / 2 + 1));
    show("extent_max_2", vb_extent_ok(big, 2));

    // byte offsets of rows * ld elements (the batch-finishing calls): 2-byte binary16 rows, 4-byte fp32 rows
    const int64_t p50 = (int64_t)1 << 50, p52 = (int64_t)1 << 52;
    show("bytes_0_max_4", vb_byte_extent_ok(0, big, 4));
    show("bytes_neg_max_4", vb_byte_extent_ok(-1, big, 4));
    show("bytes_p50_2048_2", vb_byte_extent_ok(p50, 2048, 2));          // 2^62 bytes
    show("bytes_p50_2048_4", vb_byte_extent_ok(p50, 2048, 4));          // 2^63 bytes
    show("bytes_p52_2048_2", vb_byte_extent_ok(p52, 2048, 2));          // 2^63 elements: the product itself overflows
    show("bytes_1_quarter_4", vb_byte_extent_ok(1, big / 4, 4));
    show("bytes_1_quarter_plus_1_4", vb_byte_extent_ok(1, big / 4 + 1, 4));
    show("bytes_max_2_2", vb_byte_extent_ok(big, 2, 2));

    const int64_t widths[] ={0, 1, 256, 257, 30522, 1601};
    for (int64_t n : widths) {
        char name[32];
        snprintf(name, sizeof name, "padded_%lld", (long long)n);
        show(name, vb_padded256(n));
    }

    const struct { int threads; int64_t cap; } grids[] = {{256, 2048}, {256, 4096}, {8, 4096}};
    for (const auto& g : grids) {
        const int64_t full = g.cap * g.threads;
        const int64_t items[] = {0, 1, full, full + 1};
        const char* tags[] = {"0", "1", "full", "full_plus_1"};
        for (int i = 0; i < 4; ++i) {
            char name[48];
            snprintf(name, sizeof name, "grid_%d_%lld_%s", g.threads, (long long)g.cap, tags[i]);
            show(name, vb_grid_for(items[i], g.threads, g.cap));
        }
    }

    const void* aligned = g_buf;
    const void* off2 = g_buf + 2;
    show("row16_aligned_8", vb_row16_ok(aligned, 8));
    show("row16_aligned_12", vb_row16_ok(aligned, 12));
    show("row16_off2_8", vb_row16_ok(off2, 8));
    show("row16_off2_12", vb_row16_ok(off2, 12));
    show("row32_aligned_4", vb_row32_ok(aligned, 4));
    show("row32_aligned_6", vb_row32_ok(aligned, 6));
    show("row32_off2_4", vb_row32_ok(off2, 4));
    show("row32_off2_6", vb_row32_ok(off2, 6));
    return 0;
}
