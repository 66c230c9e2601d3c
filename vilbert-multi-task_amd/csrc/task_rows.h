// Which packed rows a sample of a fine-tuning batch owns (include/vilbert_hip_task_inputs.h; task_batch.hip): the ONE function
// from the device-resident `offsets` / `mean_rows` words to a span inside [0, total_rows]. The words cannot be validated without
// a synchronisation, so every kernel clamps them through this function BEFORE it forms an address: whatever they hold, no row
// outside the packed arrays is read.
// Plain C++ without a HIP header: tests/task_rows_driver.cpp compiles it with the host compiler (and its sanitizers); device
// code gets the same function as __host__ __device__.
#pragma once
#include <stdint.h>

#if defined(__HIP__)
#define VB_TASK_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define VB_TASK_FN static inline
#endif

namespace vbtask {

struct Span {
    int64_t start;   // first packed row of the sample, in [0, total_rows]
    int64_t rows;    // n_b, in [0, total_rows - start]
    int64_t mean;    // leading rows that enter the mean, in [0, rows]
    int64_t kept;    // output rows that are not padding: min(rows + 1, max_regions)
};

// lo = offsets[b], hi = offsets[b + 1]; mean_rows < 0 with has_mean == false stands for "all rows". No intermediate can
// overflow: hi - start is only formed when hi > start >= 0.
VB_TASK_FN Span span(int64_t lo, int64_t hi, int64_t total_rows, bool has_mean, int32_t mean_rows, int32_t max_regions) {
    Span s;
    const int64_t N = total_rows < 0 ? 0 : total_rows;
    s.start = lo < 0 ? 0 : (lo > N ? N : lo);
    const int64_t room = N - s.start;
    s.rows = hi <= s.start ? 0 : (hi - s.start > room ? room : hi - s.start);
    s.mean = !has_mean ? s.rows : (mean_rows < 0 ? 0 : (mean_rows > s.rows ? s.rows : (int64_t)mean_rows));
    const int64_t R = max_regions < 1 ? 1 : max_regions;
    s.kept = s.rows + 1 < R ? s.rows + 1 : R;
    return s;
}

}  // namespace vbtask
