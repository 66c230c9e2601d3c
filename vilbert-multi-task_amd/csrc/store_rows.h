// Which rows of a device-resident region store an output sample of a batch owns (include/vilbert_hip_store.h;
// region_store.hip): the ONE path from the device-resident `image_ids` / `image_offsets` / `mean_rows` words to a span inside
// [0, total_rows]. None of the words can be validated without a synchronisation, so the id is validated first - an id outside
// [0, num_images) reads NO store word and owns nothing, not even the mean row (kept == 0: the sample is all padding) - and the
// words of a valid id go through the clamp of task_rows.h BEFORE any address is formed.
// Plain C++ without a HIP header: tests/store_span_driver.cpp compiles it with the host compiler (and its sanitizers) and
// passes recording arrays for `image_offsets` / `mean_rows` (anything with operator[]); device code passes the pointers.
#pragma once
#include "task_rows.h"

namespace vbstore {

// the validated image of an id word: the id itself, or -1 for anything outside [0, num_images). One unsigned comparison (a
// negative id is a huge unsigned one): with the two signed ones hipcc gives the bf16 feature kernel 130 VGPRs instead of the
// 128 of its packed twin, one wave per SIMD fewer.
VB_TASK_FN int64_t image(int64_t id, int64_t num_images) {
    const uint64_t n = num_images < 0 ? 0 : (uint64_t)num_images;
    return (uint64_t)id < n ? id : -1;
}

// the span of image `img` (what image() returned); reads image_offsets[img], image_offsets[img + 1] and, with has_mean,
// mean_rows[img] - and nothing at all for img < 0
template <typename Offsets, typename MeanRows>
VB_TASK_FN vbtask::Span span(int64_t img, const Offsets& image_offsets, bool has_mean, const MeanRows& mean_rows,
                             int64_t total_rows, int32_t max_regions) {
    if (img < 0) return vbtask::Span{0, 0, 0, 0};
    return vbtask::span(image_offsets[img], image_offsets[img + 1], total_rows, has_mean, has_mean ? mean_rows[img] : 0,
                        max_regions);
}

}  // namespace vbstore
