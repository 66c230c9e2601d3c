// Host driver of tests/test_bf16_round.py: rounds fp32 values with csrc/bf16_round.h - the definition every bf16 store of
// the library uses - on the CPU. Compiled with the host C++ compiler; no GPU, no library.
//
// stdin: raw little-endian fp32 values; stdout: one raw uint16 per value, the bits vb_bf16_round gives. Every second pair
// goes through vb_bf16_pack (the form most kernels store with), so both entry points are pinned.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bf16_round.h"

int main() {
    std::vector<float> in(1 << 16);
    std::vector<uint16_t> out(in.size());
    size_t n;
    while ((n = fread(in.data(), sizeof(float), in.size(), stdin)) > 0) {
        size_t i = 0;
        for (; i + 4 <= n; i += 4) {
            out[i] = (uint16_t)vb_bf16_round(in[i]);
            out[i + 1] = (uint16_t)vb_bf16_round(in[i + 1]);
            const uint32_t w = vb_bf16_pack(in[i + 2], in[i + 3]);
            out[i + 2] = (uint16_t)w;
            out[i + 3] = (uint16_t)(w >> 16);
        }
        for (; i < n; ++i) out[i] = (uint16_t)vb_bf16_round(in[i]);
        if (fwrite(out.data(), sizeof(uint16_t), n, stdout) != n) return 1;
    }
    return 0;
}
