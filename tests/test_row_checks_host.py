"""The host-side argument checks and launch arithmetic of the row kernels (csrc/row_checks.h: vb_extent_ok, vb_byte_extent_ok, vb_padded256,
vb_grid_for, vb_row16_ok / vb_row32_ok - what every vbh_ / vbf_ / vbt_ / vbp_ entry point tests before it launches) at their
boundaries, through the stand-alone tests/row_checks_driver.cpp - built with the host compiler's address and
undefined-behaviour sanitizers where it has them (the int64 products of vb_extent_ok and vb_grid_for must not overflow)."""
import os
import subprocess

import pytest

from test_gemm_plan import CSRC, TESTS, host_compiler

DRIVER = os.path.join(TESTS, "row_checks_driver.cpp")


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    work = str(tmp_path_factory.mktemp("rowchecks"))
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, DRIVER]
    exe = os.path.join(work, "row_checks_driver_san")
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe], capture_output=True)
    if san.returncode != 0:          # (a compiler without the sanitizer runtimes: the plain build still checks the values)
        exe = os.path.join(work, "row_checks_driver")
        subprocess.run(base + ["-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return dict((n, int(v)) for n, v in (line.split("\t") for line in out.splitlines()))


def test_extent_fits_int64(cases):
    got = {k[len("extent_"):]: v for k, v in cases.items() if k.startswith("extent_")}
    assert got == {"0_max": 1, "neg_max": 1, "1_max": 1, "2_half": 1, "2_half_plus_1": 0, "max_2": 0}


def test_byte_extent_fits_int64(cases):
    """vb_byte_extent_ok(rows, ld, bytes per element): the one check of the batch-finishing calls (batch.hip, task_batch.hip,
    mask_batch.hip) - the element count and its byte offset both stay inside int64, and neither product overflows on the way."""
    got = {k[len("bytes_"):]: v for k, v in cases.items() if k.startswith("bytes_")}
    assert got == {"0_max_4": 1, "neg_max_4": 1, "p50_2048_2": 1, "p50_2048_4": 0, "p52_2048_2": 0, "1_quarter_4": 1,
                   "1_quarter_plus_1_4": 0, "max_2_2": 0}


def test_padded_width(cases):
    got = {int(k[len("padded_"):]): v for k, v in cases.items() if k.startswith("padded_")}
    assert got == {0: 0, 1: 256, 256: 256, 257: 512, 30522: 30720, 1601: 1792}


def test_grid_is_capped_and_never_empty(cases):
    for threads, cap in ((256, 2048), (256, 4096), (8, 4096)):
        got = [cases["grid_%d_%d_%s" % (threads, cap, tag)] for tag in ("0", "1", "full", "full_plus_1")]
        assert got == [1, 1, cap, cap]


def test_rows_addressable_by_16_byte_accesses(cases):
    got = {k: v for k, v in cases.items() if k.startswith("row")}
    assert got == {"row16_aligned_8": 1, "row16_aligned_12": 0, "row16_off2_8": 0, "row16_off2_12": 0,
                   "row32_aligned_4": 1, "row32_aligned_6": 0, "row32_off2_4": 0, "row32_off2_6": 0}
