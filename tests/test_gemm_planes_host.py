"""tests/planes_restatement.py on the CPU: what the direct GPU tests of the bf16-plane GEMM kernel (tests/test_gemm_planes_gpu.py)
take for granted.

  * the plane split is exact: x0 + x1 + x2 == x bit for bit with three planes on normal-range values (and x0 + x1 (+ x2)
    never moves further from x than one rounding of the last plane);
  * the restated arithmetic of every mode, in float64, stays under a FIFTH of that mode's bound (tests/test_gemm_modes_gpu.py
    _check: 3e-5 / 6e-4 / 2^-6 of max(1, max|want|)) on the operands of every problem the GPU tests run (both input families).
    That is the condition under which a GPU failure means the kernel and not the inputs: the kernel's fp32 accumulation adds
    about 4e-7 of the same scale;
  * the restated tile census and split counts equal csrc/gemm_plan.h's (compiled for the host: tests/planes_census_driver.cpp)
    on every launch the GPU tests assert them for, and the shape table's recorded census equals both.
"""
import os
import shutil
import subprocess

import pytest
import torch

import planes_restatement as PR

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "vilbert-multi-task_amd", "csrc")
MODES = ("bf16x6", "bf16x3", "bf16", "f32")


def test_three_planes_are_exact_on_normal_range_values():
    g = torch.Generator().manual_seed(11)
    # magnitudes from 2^-40 to 2^40 (three bf16 planes hold 24 significand bits as long as the last plane stays normal:
    # |x| >= 2^-126 + 16 suffices), both signs, plus exact powers of two, values one ulp around them and zeros
    x = torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-40, 41, (1 << 16,), generator=g).float())
    pw = torch.exp2(torch.arange(-100, 100).float())
    x = torch.cat([x, pw, -pw, torch.nextafter(pw, torch.zeros(())), torch.nextafter(pw, torch.full((), 1e38)), torch.zeros(4)])
    p0, p1, p2 = PR.split(x, 3)
    for p in (p0, p1, p2):
        assert torch.equal(p, p.to(torch.bfloat16).float())           # every plane is a bf16 value
    assert torch.equal(((p0.double() + p1.double()) + p2.double()).float().view(torch.int32), x.view(torch.int32))
    assert torch.equal((p0 + p1) + p2, x)                              # (in fp32 too: every partial sum is representable)
    # two planes / one plane: within one rounding of the last plane kept (half a bf16 ulp of it: 2^-16 / 2^-8 relative)
    q0, q1 = PR.split(x, 2)
    assert bool(((q0.double() + q1.double() - x.double()).abs() <= x.double().abs() * 2.0 ** -16).all())
    assert bool(((PR.split(x, 1)[0].double() - x.double()).abs() <= x.double().abs() * 2.0 ** -8).all())


def test_product_lists_are_the_largest_terms():
    """6 of the 9 / 3 of the 4 plane products: every pair with i + j <= 2 / <= 1, each once, smallest first."""
    assert sorted(PR.PRODUCTS[3]) == sorted((i, j) for i in range(3) for j in range(3) if i + j <= 2)
    assert sorted(PR.PRODUCTS[2]) == sorted((i, j) for i in range(2) for j in range(2) if i + j <= 1)
    assert PR.PRODUCTS[1] == ((0, 0),)
    for planes in (2, 3):
        order = [i + j for i, j in PR.PRODUCTS[planes]]
        assert order == sorted(order, reverse=True) and PR.PRODUCTS[planes][-1] == (0, 0)


@pytest.mark.parametrize("family", list(PR.FAMILIES))
@pytest.mark.parametrize("mode", MODES)
def test_restated_arithmetic_stays_under_a_fifth_of_the_bound(mode, family):
    worst = 0.0
    for name, (fam, _m, _n, k) in PR.PROBLEMS.items():
        if fam != family:
            continue
        a, b = PR.problem(name)
        err = PR.arithmetic_error(a, b.t().contiguous(), mode)
        worst = max(worst, err)
        assert err <= PR.BOUND[mode] / 5, "%s, problem %s (contraction %d): arithmetic error %.3e of the scale" % (mode, name, k, err)
    print("%s, %s inputs: worst arithmetic error %.3e of the scale (bound %.3e)" % (mode, family, worst, PR.BOUND[mode]))
    if mode == "f32":
        assert worst == 0.0
    else:
        assert worst > 0.0          # it really is another arithmetic


def _driver(tmp_path, argv):
    cxx = shutil.which("c++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                                       if os.path.exists(p)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(tmp_path), "planes_census_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(TESTS, "planes_census_driver.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe] + [str(v) for v in argv], check=True, capture_output=True, text=True).stdout.splitlines()
    return [tuple(int(v) for v in line.split()) for line in out]


def test_tile_census_and_split_counts_equal_the_planner(tmp_path):
    argv, want = [], []
    for name, (m, n, _k, planes, f32) in PR.SHAPES.items():
        for planes_mode, recorded in ((1, planes), (0, f32)):
            assert PR.tile_census(m, n, 1, bool(planes_mode)) == recorded, name
            argv += ["t", m, n, 1, planes_mode, (m + 127) // 128 * 128]
            want.append(recorded)
    # a grid around the rule's edges: 1 .. 66 and 255 .. 258 leftover tiles, split launches, a segment size that is no
    # multiple of 64
    for tiles_n in list(range(1, 67)) + [192, 193, 255, 256, 257, 258, 320, 321]:
        for splits in (1, 4):
            for planes_mode in (0, 1):
                for cseg in (128, 96):
                    argv += ["t", 100, 128 * tiles_n, splits, planes_mode, cseg]
                    want.append(PR.tile_census(100, 128 * tiles_n, splits, bool(planes_mode), cseg))
    for tiles in (1, 2, 3, 4, 6, 12, 65, 100, 256, 300):
        for kt in (1, 3, 4, 15, 16, 17, 64, 1000):
            argv += ["w", tiles, kt]
            want.append((PR.wgrad_splits(tiles, kt),))
    for m, n, k in ((64, 64, 4096), (64, 64, 4100), (64, 64, 1023), (64, 64, 1 << 20), (1628, 768, 30522), (2048, 1024, 4096)):
        argv += ["d", m, n, k]
        want.append((PR.dgrad_splits(m, n, k),))
    assert _driver(tmp_path, argv) == want
    # the counts the GPU tests name
    assert PR.dgrad_splits(64, 64, 4096) == 4 and PR.dgrad_splits(64, 64, 4100) == 4
    assert PR.wgrad_splits(1, 16) == 4 and PR.wgrad_splits(2, 3) == 1
