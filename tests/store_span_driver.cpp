// Host driver of tests/test_region_store.py: the path from an id word of a batch to the rows of a device-resident region store
// (csrc/store_rows.h, applied by both kernels of csrc/region_store.hip before they form an address) over valid and invalid ids
// and well-formed and corrupt store words. The store's words are handed over as RECORDING arrays: every index the header forms
// is checked against [0, size) before it is served, so "an invalid id reads no store word" and "no word outside
// image_offsets[0 .. num_images] is indexed" are counted facts, with or without a sanitizer. Compiled with the host C++
// compiler (and its sanitizers where it has them); no GPU, no library. Reads nothing; prints
// "<case>\t<image>\t<start>\t<rows>\t<mean>\t<kept>\t<offset words read>\t<mean words read>" per line and checks what the
// kernels rely on itself: exit status 1 and a line on stderr where it does not hold.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "store_rows.h"

namespace {

int failures = 0;

template <typename T>
struct Recorded {
    std::vector<T> words;
    mutable long reads = 0, outside = 0;
    T operator[](int64_t i) const {
        ++reads;
        if (i < 0 || i >= (int64_t)words.size()) {
            ++outside;
            return T(0);
        }
        return words[(size_t)i];
    }
};

void fail(const char* name, const char* what) {
    fprintf(stderr, "%s: %s\n", name, what);
    ++failures;
}

// one id against a store of offsets.size() - 1 images
void show(const char* name, int64_t id, const std::vector<int64_t>& offsets, const std::vector<int32_t>& means, int64_t total,
          int32_t regions) {
    Recorded<int64_t> off;
    Recorded<int32_t> mean;
    off.words = offsets;
    mean.words = means;
    const int64_t num_images = (int64_t)offsets.size() - 1;
    const bool has_mean = !means.empty();
    const int64_t img = vbstore::image(id, num_images);
    const vbtask::Span s = vbstore::span(img, off, has_mean, mean, total, regions);
    printf("%s\t%lld\t%lld\t%lld\t%lld\t%lld\t%ld\t%ld\n", name, (long long)img, (long long)s.start, (long long)s.rows,
           (long long)s.mean, (long long)s.kept, off.reads, mean.reads);
    const int64_t N = total < 0 ? 0 : total;
    if (off.outside != 0 || mean.outside != 0) fail(name, "a word outside the store's arrays was indexed");
    if (s.start < 0 || s.rows < 0 || s.start > N || s.rows > N - s.start) fail(name, "the span leaves [0, total_rows]");
    if (s.mean < 0 || s.mean > s.rows) fail(name, "the mean count leaves [0, rows]");
    const bool valid = id >= 0 && id < num_images;
    if (img != (valid ? id : -1)) fail(name, "the validated image is not the id / -1");
    if (valid) {
        if (off.reads != 2 || mean.reads != (has_mean ? 1 : 0)) fail(name, "a valid id reads two offsets and its mean word");
        if (s.kept < 1 || s.kept > s.rows + 1) fail(name, "a valid id keeps its mean row and at most its rows");
    } else {
        if (off.reads != 0 || mean.reads != 0) fail(name, "an invalid id read a store word");
        if (s.start != 0 || s.rows != 0 || s.mean != 0 || s.kept != 0) fail(name, "an invalid id owns something");
    }
}

}  // namespace

int main() {
    const std::vector<int64_t> good = {0, 3, 4, 40, 100};          // 4 images, 100 rows
    const std::vector<int32_t> none, means = {2, 1, 36, 9};
    show("first", 0, good, none, 100, 101);
    show("last", 3, good, none, 100, 101);
    show("truncated", 2, good, none, 100, 6);
    show("one_region", 2, good, none, 100, 1);
    show("with_mean", 2, good, means, 100, 101);
    show("mean_when_truncated", 3, good, means, 100, 4);
    show("id_minus_one", -1, good, means, 100, 101);
    show("id_num_images", 4, good, means, 100, 101);
    show("id_past_num_images", 5, good, means, 100, 101);
    show("id_2_to_40", (int64_t)1 << 40, good, means, 100, 101);
    show("id_int64_max", INT64_MAX, good, means, 100, 101);
    show("id_int64_min", INT64_MIN, good, means, 100, 101);
    show("id_minus_one_as_u32", 0xFFFFFFFFll, good, none, 100, 101);
    show("empty_store", 0, {0}, none, 0, 101);
    show("empty_store_negative", -3, {0}, none, 0, 101);
    // corrupt words on the device: the clamp of task_rows.h holds whatever they say
    show("decreasing", 1, {0, 30, 20, 100}, none, 100, 101);
    show("offset_past_total", 1, {0, 90, 250, 300}, none, 100, 101);
    show("start_past_total", 2, {0, 90, 250, 300}, none, 100, 101);
    show("negative_offset", 0, {-7, 5, 100}, none, 100, 101);
    show("int64_extremes", 0, {INT64_MIN, INT64_MAX}, none, 100, 101);
    show("int64_max_both", 0, {INT64_MAX, INT64_MAX}, none, 100, 101);
    show("mean_above_rows", 1, good, {2, 40, 36, 9}, 100, 101);
    show("mean_negative", 1, good, {2, -5, 36, 9}, 100, 101);
    show("filled_part_only", 2, good, none, 40, 101);               // total_rows = the filled part of a larger allocation
    show("negative_total", 1, good, none, -4, 101);
    show("regions_not_positive", 2, good, none, 100, 0);
    return failures == 0 ? 0 : 1;
}
