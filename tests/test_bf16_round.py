"""The fp32 -> bf16 rounding of every bf16 store (csrc/bf16_round.h) on the CPU.

The header is host-only code, so this test compiles tests/bf16_round_driver.cpp against it with the host C++ compiler and
rounds every rounding DECISION: all 65,536 upper halves x the lower halves {0, 1, 0x7ffe, 0x7fff, 0x8000, 0x8001, 0xfffe,
0xffff} - below / at / above a tie with an even and with an odd kept bit, for every exponent and both signs, fp32
subnormals, bf16-subnormal results, the largest finites (which must carry into Inf), +-Inf and every NaN class.

Contract (the same one tests/test_bf16_helpers_gpu.py holds the kernels to):
  * a non-NaN input gives torch's CPU cast `x.to(torch.bfloat16)`, bit for bit;
  * a NaN input gives a bf16 NaN, quiet, with the input's sign. The add-and-shift alone gave +Inf for 0x7f800001 ..
    0x7f80ffff and -0 / +0 for 0x7fff8000 .. 0x7fffffff / 0xffff8000 .. 0xffffffff.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from helpers import check_rounding_contract, rounding_patterns, torch_cast_bits

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "vilbert-multi-task_amd", "csrc")
DRIVER = os.path.join(TESTS, "bf16_round_driver.cpp")


def host_compiler():
    return shutil.which("c++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                                        if os.path.exists(p)), None)


@pytest.fixture(scope="module")
def rounded(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(tmp_path_factory.mktemp("bf16_round")), "bf16_round_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe], check=True)
    bits = rounding_patterns()
    out = subprocess.run([exe], input=bits.astype("<u4").tobytes(), check=True, capture_output=True).stdout
    got = np.frombuffer(out, dtype="<u2").astype(np.uint16)
    assert got.size == bits.size
    return bits, got


def test_patterns_cover_every_class():
    bits = rounding_patterns()
    assert bits.size == 8 << 16 and np.unique(bits).size == bits.size
    a = bits & 0x7fffffff
    assert ((a > 0x7f800000).sum(), (a == 0x7f800000).sum()) == (2 * (127 * 8 + 7), 2)      # NaNs, infinities
    assert ((a > 0) & (a < 0x00800000)).sum() == 2 * (128 * 8 - 1)                          # fp32 subnormals
    assert ((a >= 0x7f7f8000) & (a < 0x7f800000)).sum() == 2 * 4                            # finites that round to Inf


def test_rounding_matches_torch_bit_for_bit_and_keeps_nan(rounded):
    bits, got = rounded
    nan = check_rounding_contract(bits, got, "vb_bf16_round")
    # a NaN stays a QUIET NaN of the same sign, with the upper payload bits it had
    assert ((got[nan] & 0x0040) != 0).all() and ((got[nan] >> 15) == (bits[nan] >> 31)).all()
    assert ((got[nan] | 0x0040) == ((bits[nan] >> 16) | 0x0040)).all()
    # the classes the add-and-shift alone got wrong, by value
    by_bits = dict(zip(bits.tolist(), got.tolist()))
    assert by_bits[0x7f800001] == 0x7fc0 and by_bits[0x7f80ffff] == 0x7fc0
    assert by_bits[0x7fffffff] == 0x7fff and by_bits[0xffffffff] == 0xffff and by_bits[0xffff8000] == 0xffff
    assert by_bits[0x7fc00000] == 0x7fc0 and by_bits[0x7f800000] == 0x7f80 and by_bits[0xff800000] == 0xff80
    assert by_bits[0x7f7f8000] == 0x7f80 and by_bits[0x7f7f7fff] == 0x7f7f                   # largest finites
    assert by_bits[0x00008000] == 0x0000 and by_bits[0x00008001] == 0x0001 and by_bits[0x00018000] == 0x0002  # subnormal ties


def test_contract_checker_rejects_the_old_rounding():
    """The checker the GPU tests share must fail for the add-and-shift without the NaN case (and only on NaNs)."""
    bits = rounding_patterns()
    old = ((bits.astype(np.uint64) + 0x7fff + ((bits >> 16) & 1)) >> 16).astype(np.uint16)   # (wraps like 32-bit unsigned)
    nan = (bits & 0x7fffffff) > 0x7f800000
    assert (old[~nan] == torch_cast_bits(bits)[~nan]).all()
    with pytest.raises(AssertionError, match="NaN inputs did not stay NaN"):
        check_rounding_contract(bits, old, "add-and-shift")
    assert old[bits == 0x7f800001][0] == 0x7f80 and old[bits == 0x7fffffff][0] == 0x8000 and old[bits == 0xffffffff][0] == 0
