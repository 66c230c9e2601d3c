"""The GEMM planners (csrc/gemm_plan.h) on the CPU: which kernel, tile shape and split count every launch gets.

The planners are host-only arithmetic on the problem shape, pointer alignment and the settings in PlanKnobs. This test
compiles tests/gemm_plan_driver.cpp against the header with the host C++ compiler, runs it over a fixed grid of launches
(the model's linears in the three operand layouts, the MLM decoder cases, stacked q | k | v, every epilogue, weight
gradients around the split rule's fill threshold, forced settings) and compares every case with
tests/golden/gemm_plans.json - exactly. The golden file was recorded when the planners were moved out of gemm.hip
unchanged, so it states the decisions the kernels were tuned and measured with: an edit of the planner code that changes
an entry is a bug (or a deliberate re-tuning, which then regenerates the file and says so):

    python tests/test_gemm_plan.py --write      # rewrites tests/golden/gemm_plans.json

The file holds one row per (family, layout, M x N, ...) with one entry per K; flat, a case is "<id>": "<result>". id = family (g grid, d decoder, q stacked q | k | v, w fill threshold, e epilogues, f
forced), layout, M x N x K of the launch as the kernels see it (TN: dW rows x in-features x contraction rows), then
what differs from the layout's usual launch: epilogue (store; TN atomic), splits (1; TN -1 = planner's choice),
nseg, lda, the forced setting. result, space separated:
    plan_v2         "-" refused, else tm1,tm2,tn,big_rows,small_rows,tiles_n,splits,kt_per_split,cost (hex float)
    v4:a,b,c,d      plan_v4's code under modes 0, 1, 2 and under mode 1 with VB_GEMM_V4_SMALLM (NT / NN, unsplit)
    w1: w2:         plan_v4w under modes 1, 2: cfg,tiles_n,n_small,n_big,ktiles_per_split,epi ("=": same as w1)
    t:a,b/c,d       plan_tiles n_big,n_small for the fp32 kernel / the bf16-planes kernel
    ws: ds:         round-1 weight-gradient split count (TN); bf16-plane split-K dgrad count (NN)
"""
import json
import os
import shutil
import subprocess
import sys

import pytest

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "vilbert-multi-task_amd", "csrc")
DRIVER = os.path.join(TESTS, "gemm_plan_driver.cpp")
GOLDEN = os.path.join(TESTS, "golden", "gemm_plans.json")
ROWS, FEAT = (1628, 2304, 2368, 9216, 9472, 18432), (768, 1024, 2048, 2304, 3072, 4096)
EPILOGUES = ("generic", "store", "gelu", "res", "pre_gelu", "accum", "atomic", "res_drop", "dgelu", "mul")


def host_compiler():
    return shutil.which("c++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++")
                                        if os.path.exists(p)), None)


def run_driver(workdir):
    """Compile the driver in `workdir` and return its cases {id: result}, in the driver's order."""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(workdir), "gemm_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe], check=True)
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert lines[0] == "sizeof(GemmP)\t360"   # recorded from the parent commit: the struct is a kernel argument
    cases = dict(line.split("\t") for line in lines[1:])
    assert len(cases) == len(lines) - 1, "two cases of the driver share an id"
    assert flat(table(cases)) == cases
    return cases


def table(cases):
    """{id: result} -> the golden file's layout {id without K: {K: result}} (one row of the file per M x N)."""
    rows = {}
    for cid, res in cases.items():
        fam, layout, dims, *rest = cid.split()
        mn, k = dims.rsplit("x", 1)
        rows.setdefault(" ".join([fam, layout, mn] + rest), {})[k] = res
    return rows


def flat(rows):
    out = {}
    for rid, by_k in rows.items():
        fam, layout, mn, *rest = rid.split()
        for k, res in by_k.items():
            out[" ".join([fam, layout, "%sx%s" % (mn, k)] + rest)] = res
    return out


def test_header_is_host_only(tmp_path):
    """gemm_plan.h compiles alone with the host compiler: no HIP header, and no environment reads of its own."""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    src = tmp_path / "only.cpp"
    src.write_text('#include "gemm_plan.h"\n')
    subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)], check=True)
    assert "getenv" not in open(os.path.join(CSRC, "gemm_plan.h")).read()


def test_plans_match_golden(tmp_path):
    got = run_driver(tmp_path)
    with open(GOLDEN) as f:
        want = flat(json.load(f))
    assert sorted(got) == sorted(want), "the driver's grid and the golden file's differ"
    wrong = [k for k in want if want[k] != got[k]]
    for k in wrong[:10]:
        print("%s\n  golden: %s\n     got: %s" % (k, want[k], got[k]))
    assert not wrong, "%d of %d planner decisions changed" % (len(wrong), len(want))


def test_grid_covers_the_model():
    """The golden file holds the whole grid: layouts x rows x features, decoder, stacked q | k | v, epilogues, forced."""
    with open(GOLDEN) as f:
        cases = flat(json.load(f))
    ids = set(cases)
    for m in ROWS:
        for n in FEAT:
            for k in FEAT:
                assert {"g NT %dx%dx%d" % (m, n, k), "g NN %dx%dx%d" % (m, n, k), "g TN %dx%dx%d" % (n, k, m)} <= ids
    assert sum(i.startswith("g ") for i in ids) == 3 * 6 * 6 * 6
    for kk in (30522, 30512):
        assert "d NN 1628x768x%d lda=30522" % kk in ids and "d NN 1628x768x%d accum splits=-1 lda=30522" % kk in ids
    assert "d TN 30522x768x1628 lda=30524" in ids and "d TN 30522x768x1616 lda=30524" in ids
    for seg in (768, 1024):
        for m in ROWS:
            assert {"q NT %dx%dx%d nseg=3" % (m, 3 * seg, seg), "q NN %dx%dx%d nseg=3" % (m, seg, 3 * seg),
                    "q TN %dx%dx%d nseg=3" % (3 * seg, seg, m)} <= ids
    for epi in EPILOGUES:   # (the id leaves the layout's usual epilogue out)
        assert any(i.startswith("e NT 9216x3072x768") and (epi in i.split() or epi == "store") for i in ids)
        assert any(i.startswith("e NN 9216x3072x768") and (epi in i.split() or epi == "store") for i in ids)
        assert any(i.startswith("e TN 3072x768x9216") and (epi in i.split() or epi == "atomic") for i in ids)
    assert sum(i.startswith("e ") for i in ids) == 10 * (1 + 2 + 2)
    for setting in ["tile_code=%d" % t for t in (22, 33, 34, 43, 44, 434, 433, 324, 323, -1)] + \
                   ["v4_force_cfg=%d" % t for t in (6304, 6303, 6204, 6104, 6103, 4202, 4104, 4544, 4543)]:
        assert any(i.endswith(" " + setting) for i in ids), setting
    # every decision path is present: accepted and refused by plan_v2, persistent kernels taken and not taken
    res = [r.split() for r in cases.values()]
    assert any(r[0] == "-" for r in res) and any(r[0] != "-" for r in res)
    v4 = [f[3:].split(",")[1] for r in res for f in r if f.startswith("v4:")]
    w1 = [f[3:].split(",")[0] for r in res for f in r if f.startswith("w1:")]
    assert "0" in v4 and any(c != "0" for c in v4) and "-1" in w1 and any(c != "-1" for c in w1)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        recorded = run_driver(d)
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table(recorded).items()) + "\n}\n")
    print("wrote %d cases to %s" % (len(recorded), GOLDEN))
