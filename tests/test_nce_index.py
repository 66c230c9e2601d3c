"""Host side of the native NCE region loss (visual_target == 2; csrc/nce_index.h, csrc/nce.hip, include/vilbert_hip_pretrain.h):

  * tests/nce_restatement.py equals csrc/nce_index.h compiled for the host (tests/nce_index_driver.cpp) bit for bit - a grid of
    (B, R, n_across, n_inside, g, seed) with top-bit seeds, a registered step counter, n_across == 0, n_inside == 0 - and the
    header's restated hash equals rng.h's;
  * the law of the reference's sampler (vilbert.py:1532-1557): an across negative never lies in its own sample, an inside
    negative is never its own region and always lies in its own sample, every permitted value occurs;
  * the header, its ctypes mirror and the built library agree; argument errors come back without a GPU.
No compute is launched here; the GPU side is tests/test_nce_loss_gpu.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import dropout_restatement as DR
import nce_restatement as NR
from test_dropout_mask import host_compiler

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "vilbert-multi-task_amd", "csrc")
DRIVER = os.path.join(TESTS, "nce_index_driver.cpp")
HEADER = os.path.join(ROOT, "include", "vilbert_hip_pretrain.h")
ENTRY_POINTS = ["vbp_nce_bwd", "vbp_nce_fwd", "vbp_nce_negatives", "vbp_nce_workspace"]
BADARG, RANGE = -1, -3
M64 = (1 << 64) - 1

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
            "float": ctypes.c_float, "int": ctypes.c_int}
IN = [("seed", "<u8"), ("epoch", "<u8"), ("g", "<i8"), ("batch", "<i4"), ("regions", "<i4"), ("n_across", "<i4"),
      ("n_inside", "<i4"), ("j", "<i4"), ("use_epoch", "<i4")]
OUT = [("row", "<i8"), ("hash_nce", "<u4"), ("hash_rng", "<u4")]

SEEDS = (0, 1, 0x0123456789ABCDEF, 1 << 63, M64, 0xD1B54A32D192ED03)
SHAPES = ((2, 2, 1, 0), (2, 2, 0, 1), (2, 2, 2, 1), (3, 4, 5, 3), (5, 7, 89, 38), (256, 36, 89, 38), (256, 36, 178, 76),
          (7, 1, 4, 0), (1, 9, 0, 4), (70000, 36, 3, 2))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    exe = os.path.join(str(tmp_path_factory.mktemp("nce")), "nce_index_driver")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, DRIVER, "-o", exe], check=True)

    def run(rec):
        out = subprocess.run([exe], input=rec.tobytes(), check=True, capture_output=True).stdout
        got = np.frombuffer(out, dtype=OUT)
        assert got.size == rec.size
        return got
    return run


def _records(batch, regions, n_across, n_inside, seed, regions_g, epoch=None):
    n_neg = n_across + n_inside
    g = np.repeat(np.asarray(regions_g, dtype=np.int64), n_neg)
    rec = np.zeros(g.size, dtype=IN)
    rec["seed"], rec["g"], rec["j"] = np.uint64(seed), g, np.tile(np.arange(n_neg, dtype=np.int32), len(regions_g))
    rec["batch"], rec["regions"], rec["n_across"], rec["n_inside"] = batch, regions, n_across, n_inside
    if epoch is not None:
        rec["epoch"], rec["use_epoch"] = np.uint64(epoch), 1
    return rec


def _some_regions(batch, regions):
    n = batch * regions
    edge = {0, 1, regions - 1, regions, n - regions, n - 1, n // 2}
    rng = np.random.default_rng(n)
    return sorted(g for g in edge | set(rng.integers(0, n, 24).tolist()) if 0 <= g < n)


def test_restatement_equals_the_header_bit_for_bit(driver):
    checked = 0
    for batch, regions, n_across, n_inside in SHAPES:
        gs = _some_regions(batch, regions)
        for seed in SEEDS:
            for epoch in (None, 0, 3, (1 << 64) - 5):
                got = driver(_records(batch, regions, n_across, n_inside, seed, gs, epoch))
                want = NR.negatives(seed, gs, batch, regions, n_across, n_inside, epoch)
                assert np.array_equal(got["row"].reshape(want.shape), want), (batch, regions, n_across, n_inside, seed, epoch)
                assert want.min() >= 0 and want.max() < batch * regions
                checked += want.size
    assert checked > 200000
    # a registered counter holding 0 is the host seed alone; another value moves the negatives
    a = NR.negatives(77, [5], 5, 7, 89, 38)
    assert np.array_equal(a, NR.negatives(77, [5], 5, 7, 89, 38, epoch=0))
    assert not np.array_equal(a, NR.negatives(77, [5], 5, 7, 89, 38, epoch=1))


def test_the_headers_hash_is_rng_h_vb_hash(driver):
    rng = np.random.default_rng(5)
    rec = np.zeros(4096, dtype=IN)
    rec["seed"] = rng.integers(0, 1 << 63, rec.size, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    rec["seed"][::2] |= np.uint64(1 << 63)
    rec["g"] = rng.integers(0, 1 << 62, rec.size, dtype=np.int64)
    rec["batch"], rec["regions"], rec["n_across"], rec["n_inside"] = 2, 2, 1, 1
    got = driver(rec)
    assert np.array_equal(got["hash_nce"], got["hash_rng"])
    assert np.array_equal(got["hash_nce"], DR.vb_hash(rec["seed"], rec["g"].astype(np.uint64)))


def test_the_law_of_the_references_sampler():
    B, R, n_across, n_inside = 3, 4, 40, 24
    gs = np.arange(B * R)
    seen_across = {g: set() for g in gs}
    seen_inside = {g: set() for g in gs}
    for seed in range(1, 41):
        neg = NR.negatives(seed * 0x9E3779B1 + (seed << 60), gs, B, R, n_across, n_inside)
        b, r = (gs // R)[:, None], (gs % R)[:, None]
        across, inside = neg[:, :n_across], neg[:, n_across:]
        assert (across // R != b).all() and (across >= 0).all() and (across < B * R).all()
        assert (inside // R == b).all() and (inside % R != r).all()
        for g in gs:
            seen_across[g].update(across[g].tolist())
            seen_inside[g].update(inside[g].tolist())
    for g in gs:
        b, r = divmod(int(g), R)
        assert seen_across[g] == {x for x in range(B * R) if x // R != b}, g
        assert seen_inside[g] == {b * R + c for c in range(R) if c != r}, g
    # no draw is shared between two regions or two positions: rows of one launch differ
    neg = NR.negatives(9, gs, B, R, n_across, n_inside)
    assert len({tuple(row) for row in neg.tolist()}) == B * R
    # n_across == 0 / n_inside == 0 keep the other kind's draws where they were in the stream of (g, j)
    assert NR.negatives(9, gs, B, R, 0, 5).shape == (B * R, 5) and NR.negatives(9, gs, B, R, 5, 0).shape == (B * R, 5)


def _prototypes():
    """name -> (return ctype, [argument ctypes]) parsed from the header text; every pointer is a plain address."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else _C_TYPES[a.replace("const ", "").split()[0]])
        out[name] = (_C_TYPES[ret], types)
    return out


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from vilbert import _native
    return _native


def test_header_declares_exactly_the_four_entry_points_and_stays_out_of_the_pinned_lists():
    assert sorted(_prototypes()) == ENTRY_POINTS
    text = open(HEADER).read()
    assert "vbt" + "_" not in text
    for name in ("vilbert_hip.h", "vilbert_hip_ext.h", "vilbert_hip_optim.h", "vilbert_hip_tasks.h"):
        assert "vbp_" not in open(os.path.join(ROOT, "include", name)).read(), name
    # nce_index.h is host-compilable: nothing of HIP is included
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(CSRC, "nce_index.h")).read()).replace("__HIP__", "").lower()


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes()
    assert sorted(native.PRETRAIN_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.PRETRAIN_SIGNATURES[name][0] is res, name
        assert native.PRETRAIN_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbp_[a-z0-9_]+)", nm))) == ENTRY_POINTS
    lib = native.lib()
    assert lib.vb_abi_version() == 18
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes == native.PRETRAIN_SIGNATURES[name][1]


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    a = ctypes.c_void_p(64)          # fake non-null addresses: the argument checks come before any launch
    # vbp_nce_negatives(stream, rows, region_idx, batch, regions, n_across, n_inside, seed, neg_idx)
    neg = lib.vbp_nce_negatives
    assert neg(None, 4, None, 5, 7, 2, 1, 9, a) == BADARG
    assert neg(None, 4, a, 5, 7, 2, 1, 9, None) == BADARG
    assert neg(None, -1, a, 5, 7, 2, 1, 9, a) == BADARG                     # negative rows
    assert neg(None, 4, a, 5, 7, 0, 0, 9, a) == BADARG                      # n_neg < 1
    assert neg(None, 4, a, 5, 7, -1, 3, 9, a) == BADARG and neg(None, 4, a, 5, 7, 3, -1, 9, a) == BADARG
    assert neg(None, 4, a, 1, 7, 2, 1, 9, a) == BADARG                      # an across negative needs a second sample
    assert neg(None, 4, a, 5, 1, 2, 1, 9, a) == BADARG                      # an inside negative needs a second region
    assert neg(None, 4, a, 0, 7, 0, 1, 9, a) == BADARG and neg(None, 4, a, 5, 0, 1, 0, 9, a) == BADARG
    assert neg(None, 1 << 62, a, 5, 7, 2, 1, 9, a) == RANGE                 # rows * n_neg beyond int64
    assert neg(None, 0, a, 5, 7, 2, 1, 9, a) == 0                           # nothing to do: no launch
    assert neg(None, 0, a, 1, 7, 0, 1, 9, a) == 0 and neg(None, 0, a, 5, 1, 1, 0, 9, a) == 0   # the unused kind needs nothing
    # vbp_nce_fwd(stream, rows, dim, n_neg, predict, ldp, table, table_rows, ldt, pos_idx, neg_idx, valid, count, workspace,
    #             loss, dsave, lds)
    fwd = lib.vbp_nce_fwd
    good = [None, 4, 8, 3, a, 8, a, 35, 8, a, a, a, a, a, a, a, 8]
    for pos in (4, 6, 9, 10, 12, 13, 14):                     # each required pointer null in turn
        args = list(good)
        args[pos] = None
        assert fwd(*args) == BADARG, pos
    for pos, bad in ((1, -1), (2, 0), (2, -3), (3, 0), (7, 0), (5, 7), (8, 7), (16, 7)):
        args = list(good)
        args[pos] = bad
        assert fwd(*args) == BADARG, (pos, bad)
    for pos, bad in ((3, 4096), (5, 1 << 62), (8, 1 << 62), (16, 1 << 62)):
        args = list(good)
        args[pos] = bad
        assert fwd(*args) == RANGE, (pos, bad)
    assert fwd(*[None, 0] + good[2:]) == 0                                  # no rows: no launch
    args = list(good)
    args[1], args[11], args[15], args[16] = 0, None, None, 0                # valid and dsave are optional
    assert fwd(*args) == 0
    # vbp_nce_bwd(stream, rows, dim, dsave, lds, valid, grad_loss, count, dpredict, ldd)
    bwd = lib.vbp_nce_bwd
    good = [None, 4, 8, a, 8, a, a, a, a, 8]
    for pos in (3, 6, 7, 8):
        args = list(good)
        args[pos] = None
        assert bwd(*args) == BADARG, pos
    for pos, bad in ((1, -1), (2, 0), (4, 7), (9, 7)):
        args = list(good)
        args[pos] = bad
        assert bwd(*args) == BADARG, (pos, bad)
    for pos in (4, 9):
        args = list(good)
        args[pos] = 1 << 62
        assert bwd(*args) == RANGE, pos
    assert bwd(None, 0, 8, a, 8, None, a, a, a, 8) == 0


def test_workspace_is_one_float_per_block_of_the_forward(native):
    ws = native.lib().vbp_nce_workspace
    assert ws(0) == 0 and ws(-3) == 0 and ws(1) == 1 and ws(1380) == 1380 and ws(4096) == 4096 and ws(1 << 40) == 4096


def test_cpu_tensors_and_the_switch_keep_the_reference_shaped_loss(monkeypatch):
    """The native path needs fp32 HIP tensors, two samples and two regions: everything else (and VB_NCE_NATIVE=0) leaves
    visual_target == 2 with _nce_region_loss; _static_gather() no longer looks at the visual target."""
    import inspect

    import torch
    from oracle import synth
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    m = BertForMultiModalPreTraining(BertConfig.from_dict(synth.tiny_config(visual_target=2, v_target_size=48)))
    assert m.visual_target == 2 and m._nce_seed is None
    assert not m._nce_native(torch.zeros(4, 9, 8), torch.zeros(4, 8, 48))
    # (the meta device stands in for a HIP device: only properties are read)
    feat, target = torch.zeros(4, 9, 8, device="meta"), torch.zeros(4, 8, 48, device="meta")
    native = lambda f, t: m._nce_native(_as_cuda(f), _as_cuda(t))
    assert native(feat, target)
    assert not native(feat, target.double()) and not native(feat.half(), target)
    assert not native(feat[:1], target[:1]) and not native(feat, target[:, :1])
    assert not native(feat, torch.zeros(4, 8, 48, device="meta", requires_grad=True))
    monkeypatch.setenv("VB_NCE_NATIVE", "0")
    assert not native(feat, target)
    monkeypatch.delenv("VB_NCE_NATIVE")
    m.visual_target = 0
    assert not native(feat, target)
    assert "visual_target" not in inspect.getsource(BertForMultiModalPreTraining._static_gather)


class _as_cuda(object):
    """A tensor's properties with is_cuda forced on (no GPU here)."""

    def __init__(self, t):
        self._t = t
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self._t, name)
