// Host driver of tests/test_task_batch.py: the clamp of a sample's span in a packed fine-tuning batch (csrc/task_rows.h, applied
// by every kernel of csrc/task_batch.hip before it forms an address) over well-formed and malformed offsets. Compiled with the
// host C++ compiler (and its sanitizers where it has them); no GPU, no library. Reads nothing; prints
// "<case>\t<start>\t<rows>\t<mean>\t<kept>" per line; all checking is done by the test.
#include <stdint.h>
#include <stdio.h>

#include "task_rows.h"

namespace {

void show(const char* name, int64_t lo, int64_t hi, int64_t total, bool has_mean, int32_t mean, int32_t regions) {
    const vbtask::Span s = vbtask::span(lo, hi, total, has_mean, mean, regions);
    printf("%s\t%lld\t%lld\t%lld\t%lld\n", name, (long long)s.start, (long long)s.rows, (long long)s.mean, (long long)s.kept);
}

}  // namespace

int main() {
    show("plain", 10, 25, 100, false, 0, 101);
    show("plain_mean", 10, 25, 100, true, 12, 101);
    show("truncated", 10, 25, 100, false, 0, 6);
    show("exactly_full", 10, 15, 100, false, 0, 6);
    show("one_region", 10, 25, 100, false, 0, 1);
    show("empty_sample", 10, 10, 100, false, 0, 6);
    show("negative_start", -7, 5, 100, false, 0, 6);
    show("negative_both", -7, -3, 100, false, 0, 6);
    show("decreasing", 30, 20, 100, false, 0, 6);
    show("end_too_large", 90, 250, 100, false, 0, 101);
    show("start_too_large", 150, 160, 100, false, 0, 101);
    show("start_at_end", 100, 104, 100, false, 0, 101);
    show("int64_extremes", INT64_MIN, INT64_MAX, 100, false, 0, 101);
    show("int64_max_both", INT64_MAX, INT64_MAX, 100, false, 0, 101);
    show("int64_min_end", 5, INT64_MIN, 100, false, 0, 101);
    show("mean_above_rows", 10, 25, 100, true, 40, 101);
    show("mean_negative", 10, 25, 100, true, -2, 101);
    show("mean_zero", 10, 25, 100, true, 0, 101);
    show("mean_with_clamped_rows", 95, 250, 100, true, 9, 101);
    show("no_rows_at_all", 0, 5, 0, true, 3, 6);
    show("negative_total", 0, 5, -4, false, 0, 6);
    show("regions_not_positive", 10, 25, 100, false, 0, 0);
    return 0;
}
