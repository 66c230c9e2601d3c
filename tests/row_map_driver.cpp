// Host driver of tests/test_row_map_host.py: the validation of an output + feed-forward block's row map (csrc/row_map.h,
// called by vb_layer_fwd / vb_layer_bwd) over accepted and refused argument sets. Compiled with the host C++ compiler (and
// its sanitizers where it has them); no GPU, no library. Prints "<case>\t<code>" per line; all checking is done by the test.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "row_map.h"

namespace {

alignas(16) char g_buf[64];

vb_ffn_block good() {
    vb_ffn_block f;
    memset(&f, 0, sizeof f);
    f.M = 2304; f.Hc = 768; f.H = 768; f.I = 3072; f.src_rows = 9216;
    void* p = g_buf;
    f.row_map = reinterpret_cast<const int32_t*>(g_buf);
    f.ctx = p; f.x = p; f.ctx_rows = p; f.sum1 = p; f.a1 = p; f.h = p; f.sum2 = p; f.dy = p;
    f.d_ctx = p; f.d_sum1 = p; f.d_sum2 = p; f.d_sum2_drop = p; f.d_pre = p; f.d_a1 = p; f.d_sum1_drop = p;
    f.d_ctx_full = p; f.d_sum1_full = p; f.full_ws = reinterpret_cast<float*>(g_buf);
    return f;
}

void show(const char* name, const vb_ffn_block& f, bool b16, bool backward) {
    printf("%s\t%d\n", name, vbrows::check_row_map(f, b16, backward));
}

}  // namespace

int main() {
    vb_ffn_block f = good();
    show("good_fwd", f, false, false);
    show("good_bwd", f, false, true);
    show("bf16", f, true, false);
    f = good(); f.row_map = nullptr; f.src_rows = -5; show("no_map_ignores_the_rest", f, true, true);
    f = good(); f.ctx_rows = nullptr; show("no_ctx_rows", f, false, false);
    f = good(); f.src_rows = 0; show("no_src_rows", f, false, false);
    f = good(); f.src_rows = (int64_t)INT32_MAX + 1; show("src_rows_past_int32", f, false, false);
    f = good(); f.src_rows = INT32_MAX; show("src_rows_int32_max", f, false, false);
    f = good(); f.M = (int64_t)INT32_MAX + 1; show("M_past_int32", f, false, false);
    f = good(); f.M = -1; show("M_negative", f, false, false);
    f = good(); f.H = 770; show("H_not_times_4", f, false, false);
    f = good(); f.I = 3074; show("I_not_times_4", f, false, false);
    f = good(); f.H = f.Hc = 4096; show("wide", f, false, true);
    f = good(); f.H = 0; show("H_zero", f, false, false);
    f = good(); f.x = g_buf + 4; show("x_unaligned", f, false, false);
    f = good(); f.sum2 = g_buf + 8; show("sum2_unaligned", f, false, false);
    f = good(); f.d_ctx_full = nullptr; show("no_d_ctx_full_fwd", f, false, false);
    show("no_d_ctx_full_bwd", f, false, true);
    f = good(); f.d_sum1_full = nullptr; show("no_d_sum1_full_bwd", f, false, true);
    f = good(); f.d_sum1_full = g_buf + 4; show("d_sum1_full_unaligned", f, false, true);
    f = good(); f.d_sum2_drop = nullptr; f.d_sum1_drop = nullptr; show("no_dropout_twins", f, false, true);
    f = good(); f.d_sum1_drop = g_buf + 12; show("twin_unaligned", f, false, true);
    f = good(); f.full_ws = nullptr; show("no_full_ws_fwd", f, false, false);
    show("no_full_ws_bwd", f, false, true);
    f = good(); f.full_ws = reinterpret_cast<float*>(g_buf + 4); show("full_ws_unaligned", f, false, true);
    // layout of the full-size workspace: size, and 16-byte starts of every [R, .] array also for an odd row count
    const vbrows::FullWs w(9216, 768, 3072), odd(37, 96, 80);
    printf("ws_total\t%ld\n", w.total);
    printf("ws_total_odd\t%ld\n", odd.total);
    const long starts[] = {odd.dy, odd.sum2, odd.sum1, odd.a1, odd.h, odd.d_sum2, odd.d_sum2_drop, odd.d_pre, odd.d_a1, odd.d_sum1_drop};
    int misaligned = 0;
    for (long o : starts) misaligned += o % 4 != 0;
    printf("ws_misaligned\t%d\n", misaligned);
    printf("ws_tail\t%d\n", (int)(odd.stats + 4 * 37 == odd.inv && odd.inv + 37 == odd.total));
    return 0;
}
