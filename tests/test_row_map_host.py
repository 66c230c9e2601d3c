"""Host-side validation of the row map of an output + feed-forward block (csrc/row_map.h: what vb_layer_fwd / vb_layer_bwd
check before they launch the row kernels of csrc/rowmap.hip), through the stand-alone tests/row_map_driver.cpp - built with
the host compiler's address and undefined-behaviour sanitizers where it has them. The device-side part (map VALUES outside
the full tensor are padding rows) is tests/test_last_layer_rows_gpu.py's."""
import os
import re
import subprocess

import pytest

from test_gemm_plan import CSRC, TESTS, host_compiler

DRIVER = os.path.join(TESTS, "row_map_driver.cpp")
OK, BADARG, ALIGN = 0, -1, -2


def _codes():
    text = open(os.path.join(os.path.dirname(CSRC), "..", "include", "vilbert_hip.h")).read()
    return {n: int(v) for n, v in re.findall(r"#define (VB_E_[A-Z]+)\s+\(?(-\d+)\)?", text)}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    work = str(tmp_path_factory.mktemp("rowmap"))
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, DRIVER]
    exe = os.path.join(work, "row_map_driver_san")
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe], capture_output=True)
    if san.returncode != 0:          # (a compiler without the sanitizer runtimes: the plain build still checks the codes)
        exe = os.path.join(work, "row_map_driver")
        subprocess.run(base + ["-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return dict((n, int(c)) for n, c in (line.split("\t") for line in out.splitlines()))


def test_error_codes_are_the_headers():
    codes = _codes()
    assert (codes["VB_E_BADARG"], codes["VB_E_ALIGN"]) == (BADARG, ALIGN)


def test_accepted_and_refused_blocks(cases):
    want = dict(good_fwd=OK, good_bwd=OK, bf16=BADARG, no_map_ignores_the_rest=OK, no_ctx_rows=BADARG, no_src_rows=BADARG,
                src_rows_past_int32=BADARG, src_rows_int32_max=OK, M_past_int32=BADARG, M_negative=BADARG,
                H_not_times_4=ALIGN, I_not_times_4=ALIGN, wide=OK, H_zero=BADARG, x_unaligned=ALIGN, sum2_unaligned=ALIGN,
                no_d_ctx_full_fwd=OK, no_d_ctx_full_bwd=BADARG, no_d_sum1_full_bwd=BADARG, d_sum1_full_unaligned=ALIGN,
                no_dropout_twins=OK, twin_unaligned=ALIGN, no_full_ws_fwd=OK, no_full_ws_bwd=BADARG, full_ws_unaligned=ALIGN,
                ws_total=9216 * (8 * 768 + 2 * 3072 + 5), ws_total_odd=37 * (8 * 96 + 2 * 80 + 5), ws_misaligned=0, ws_tail=1)
    assert cases == want
