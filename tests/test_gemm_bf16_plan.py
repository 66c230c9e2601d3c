"""The planners of the bf16 training GEMMs (csrc/gemm_bf16_plan.h) on the CPU: block shape and persistent grid of every
forward / input-gradient launch (plan_hb), contraction splits of every weight gradient and whether it takes the deterministic
workspace slice (plan_hw).

Like tests/test_gemm_plan.py: tests/gemm_bf16_plan_driver.cpp is compiled against the header with the host C++ compiler, run
over a fixed grid and compared with tests/golden/gemm_bf16_plans.json - exactly. The golden file was recorded when the rules
were moved out of the launchers of gemm_bf16.hip unchanged, so it states the decisions the kernels were tuned and measured
with. An edit of the planner that changes an entry changes speed and the deterministic-workspace footprint: it is a bug, or
a deliberate re-tuning, which then regenerates the file and says so:

    python tests/test_gemm_bf16_plan.py --write      # rewrites tests/golden/gemm_bf16_plans.json

The file holds one row per id without its row count, with one entry per row count M. Flat, a case is "<id>": "<result>":
    hb <N>x<M> half=<VB_BF16_HALF> grid=<VB_BF16_GRID>     bm,tiles,per_cu,grid of C[M, N]
    hw <N>x<K>x<M> nseg=<n> slice=<MiB>                    splits,kt_per_split,units,grid,<ws | atomics | fallback> of
                                                           dW[N, K] (n stacked segments) from M rows
ws = partial tiles to the workspace slice + ordered reduce pass; atomics = fp32 atomics (no slice offered); fallback = a
slice was offered, not even one split fits: atomics, counted by vb_deterministic_fallbacks.
"""
import json
import os
import subprocess
import sys

import pytest

from test_gemm_plan import CSRC, TESTS, host_compiler

DRIVER = os.path.join(TESTS, "gemm_bf16_plan_driver.cpp")
GOLDEN = os.path.join(TESTS, "golden", "gemm_bf16_plans.json")
ROWS, FEAT = (1628, 2304, 2368, 9216, 9472, 18432), (768, 1024, 2304, 3072, 4096)


def build_driver(workdir):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(workdir), "gemm_bf16_plan_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe], check=True)
    return exe


def run_driver(exe, *args):
    """The driver's cases {id: result}, in the driver's order."""
    lines = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.splitlines()
    cases = dict(line.split("\t") for line in lines)
    assert len(cases) == len(lines), "two cases of the driver share an id"
    return cases


def table(cases):
    """{id: result} -> the golden file's layout {id without M: {M: result}}."""
    rows = {}
    for cid, res in cases.items():
        fam, dims, *rest = cid.split()
        shape, m = dims.rsplit("x", 1)
        rows.setdefault(" ".join([fam, shape] + rest), {})[m] = res
    return rows


def flat(rows):
    out = {}
    for rid, by_m in rows.items():
        fam, shape, *rest = rid.split()
        for m, res in by_m.items():
            out[" ".join([fam, "%sx%s" % (shape, m)] + rest)] = res
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("bf16plan"))


def test_header_is_host_only(tmp_path):
    """gemm_bf16_plan.h compiles alone with the host compiler: no HIP header, and no environment reads of its own."""
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    src = tmp_path / "only.cpp"
    src.write_text('#include "gemm_bf16_plan.h"\n')
    subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", CSRC, str(src)], check=True)
    text = open(os.path.join(CSRC, "gemm_bf16_plan.h")).read()
    assert "getenv" not in text and "vb_env" not in text and "#include <hip" not in text and "#include \"" not in text


def test_plans_match_golden(driver):
    got = run_driver(driver)
    assert flat(table(got)) == got
    with open(GOLDEN) as f:
        want = flat(json.load(f))
    assert sorted(got) == sorted(want), "the driver's grid and the golden file's differ"
    wrong = [k for k in want if want[k] != got[k]]
    for k in wrong[:10]:
        print("%s\n  golden: %s\n     got: %s" % (k, want[k], got[k]))
    assert not wrong, "%d of %d planner decisions changed" % (len(wrong), len(want))


def test_grid_covers_the_model():
    with open(GOLDEN) as f:
        cases = flat(json.load(f))
    ids = set(cases)
    for m in ROWS:
        for n in FEAT:
            for half in (0, 1, 2):
                for limit in (256, 128):
                    assert "hb %dx%d half=%d grid=%d" % (n, m, half, limit) in ids
            for k in FEAT:
                for nseg in (1, 3):
                    for mib in (0, 256, 64):
                        assert "hw %dx%dx%d nseg=%d slice=%d" % (nseg * n, k, m, nseg, mib) in ids
    assert len(ids) == 6 * 5 * 3 * 2 + 6 * 5 * 5 * 2 * 3
    # every decision path is present: both block shapes; workspace used, atomics, counted fallback; split and unsplit
    assert {cases[i].split(",")[0] for i in ids if i.startswith("hb ")} == {"256", "128"}
    assert {cases[i].split(",")[4] for i in ids if i.startswith("hw ")} == {"ws", "atomics", "fallback"}
    for i in ids:
        if i.startswith("hw "):
            assert (cases[i].split(",")[4] == "atomics") == i.endswith("slice=0"), i
    splits = {int(cases[i].split(",")[0]) for i in ids if i.startswith("hw ")}
    assert 1 in splits and max(splits) >= 8


# Split counts worked out by hand from the loop of vb_wgrad_bf16 as it stood before the planner was moved (not from the driver):
#     tiles = (N / 256) (K / 128), nkt = ceil(M / 64); candidates sp = 1 .. min(nkt, 64) with ceil(nkt / ceil(nkt / sp)) == sp,
#     per = ceil(nkt / sp), units = tiles sp, rounds = ceil(units / 256)
#     t = rounds (per t_k + 2) + units t_e                                                       without a slice
#     t = rounds (per t_k + 2) + units t_d + 3 + (sp + 2) 4 N K / 3.5e6                          with one, if sp slices fit
#     t_k = 1.0, t_e = 0.12, t_d = 0.04 (microseconds); the first candidate with the smallest t wins.
# Each case: N, K, M, slice in MiB, then the winner and its closest rival as (sp, per, units, t). Worked example, case 1:
# dW[768, 768] from 9216 rows: tiles = 3 x 6 = 18, nkt = 144. sp = 8: per 18, units 144, one round: 1 x 20 + 144 x 0.12 =
# 37.28; sp = 9: per 16, units 162: 18 + 19.44 = 37.44; sp = 7: per 21, units 126: 23 + 15.12 = 38.12 -> 8 splits. With a
# slice (case 2) a unit costs 0.04 instead of 0.12 and the reduce pass (sp + 2) x 2.36 MB / 3.5 TB/s: sp = 9: 18 + 6.48 + 3 +
# 11 x 0.674 = 34.90; sp = 12: per 12, units 216: 14 + 8.64 + 3 + 14 x 0.674 = 35.08; sp = 8: 20 + 5.76 + 3 + 6.74 = 35.50.
# Case 8: a slice of 64 MiB holds at most 3 partials of dW[1024, 4096] (16,781,312 bytes each; 4 x that = 67,125,248 >
# 67,108,864), which does not matter: 2 splits fill exactly one round. Case 12: one partial of dW[4096, 4096] is those same
# 67,125,248 bytes - no candidate fits, the launch runs unsplit on atomics and is counted.
HAND = [
    (768, 768, 9216, 0, (8, 18, 144, 37.28), (9, 16, 162, 37.44)),
    (768, 768, 9216, 256, (9, 16, 162, 34.90), (12, 12, 216, 35.08)),
    (3072, 768, 9216, 256, (3, 48, 216, 75.12), (7, 21, 504, 93.43)),
    (768, 3072, 9216, 0, (3, 48, 216, 75.92), (2, 72, 144, 91.28)),
    (1024, 1024, 2368, 256, (4, 10, 128, 27.31), (5, 8, 160, 27.79)),
    (1024, 1024, 2368, 0, (3, 13, 96, 26.52), (4, 10, 128, 27.36)),
    (2304, 768, 18432, 64, (4, 72, 216, 97.77), (9, 32, 486, 112.68)),
    (1024, 4096, 9472, 64, (2, 74, 256, 108.41), (3, 50, 384, 146.33)),
    (768, 768, 1628, 0, (3, 9, 54, 17.48), (4, 7, 72, 17.64)),
    (4096, 4096, 18432, 256, (1, 288, 512, 661.00), (2, 144, 1024, 704.66)),
    (3072, 768, 2304, 0, (2, 18, 144, 37.28), (3, 12, 216, 39.92)),
    (4096, 4096, 9216, 64, None, None),
]


def model_candidates(n, k, m, mib):
    """Every candidate of the loop described above as (t, sp, per, units), fastest first; a plain restatement in Python
    floats, not the driver."""
    tiles, nkt, out = (n // 256) * (k // 128), -(-m // 64), []
    for sp in range(1, min(nkt, 64) + 1):
        per = -(-nkt // sp)
        if -(-nkt // per) != sp:
            continue
        units = tiles * sp
        t = -(-units // 256) * (per * 1.0 + 2.0)
        if mib:
            if sp * (tiles * 32768 + n) * 4 > mib << 20:
                continue
            t += units * 0.04 + 3.0 + (sp + 2) * 4.0 * n * k / 3.5e6
        else:
            t += units * 0.12
        out.append((t, sp, per, units))
    return sorted(out)


def test_hand_table_names_the_two_fastest_candidates():
    """The table checks itself: over ALL candidates of a case, the stated winner is the fastest and the stated rival the
    second fastest, at the stated times; every other candidate is slower than the rival."""
    for n, k, m, mib, win, rival in HAND:
        cands = model_candidates(n, k, m, mib)
        if win is None:
            assert cands == []
            continue
        assert len(cands) >= 3
        for (t, sp, per, units), stated in zip(cands, (win, rival)):
            assert (sp, per, units) == stated[:3] and abs(t - stated[3]) < 0.006, (n, k, m, mib, cands[:3])
        assert cands[2][0] > cands[1][0]


def test_split_counts_worked_out_by_hand(driver):
    args = []
    for n, k, m, mib, _, _ in HAND:
        args += ["hw", n, k, m, mib << 20]
    got = run_driver(driver, *args)
    assert len(got) == len(HAND)
    for (n, k, m, mib, win, rival), (cid, res) in zip(HAND, got.items()):
        assert cid == "hw %dx%dx%d bytes=%d" % (n, k, m, mib << 20)
        splits, per, units, grid, how = res.split(",")
        if win is None:
            assert (splits, how) == ("1", "fallback") and ((n // 256) * (k // 128) * 32768 + n) * 4 > mib << 20
            continue
        for sp, kt, u, t in (win, rival):   # the stated times are the model's (the winner's margin dwarfs fp32 rounding)
            assert u == (n // 256) * (k // 128) * sp and kt == -(-(-(-m // 64)) // sp)
            model = -(-u // 256) * (kt + 2.0) + (u * 0.04 + 3.0 + (sp + 2) * 4.0 * n * k / 3.5e6 if mib else u * 0.12)
            assert abs(model - t) < 0.006, (cid, sp, model)
        assert win[3] + 0.1 < rival[3]
        assert (int(splits), int(per), int(units)) == win[:3], (cid, res)
        assert how == ("ws" if mib else "atomics") and int(grid) == min(256, (win[2] + 7) // 8 * 8)


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        recorded = run_driver(build_driver(d))
    with open(GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in table(recorded).items()) + "\n}\n")
    print("wrote %d cases to %s" % (len(recorded), GOLDEN))
