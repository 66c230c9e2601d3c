"""Host side of the device-side fine-tuning batch builder (csrc/task_batch.hip; vilbert.task_pipeline): the header
include/vilbert_hip_task_inputs.h, its ctypes mirror and the built library agree, argument errors come back without a GPU, the
numpy restatement (tests/task_batch_restatement.py) - the thing the kernels are held to bit for bit in
tests/test_task_batch_gpu.py - equals what the reference's own datasets produced (tests/golden/task_batch.npz) EXACTLY, its
column sum is numpy's, the packer round-trips, and the span clamp of csrc/task_rows.h holds for malformed offsets (through the
stand-alone tests/task_rows_driver.cpp, built with the host compiler's sanitizers where it has them). No compute is launched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import task_batch_restatement as tr
from test_gemm_plan import CSRC, TESTS, host_compiler

ROOT = os.path.dirname(TESTS)
HEADER = os.path.join(ROOT, "include", "vilbert_hip_task_inputs.h")
GOLDEN = os.path.join(TESTS, "golden", "task_batch.npz")
DRIVER = os.path.join(TESTS, "task_rows_driver.cpp")
BADARG, ALIGN, RANGE = -1, -2, -3

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototypes(native=None):
    """name -> (return ctype, [argument ctypes]) parsed from the header text; a pointer is a plain address, except the pointer to
    the argument struct, which the mirror types."""
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbd_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            if "vbd_task_batch*" in a:
                types.append(ctypes.POINTER(native.TaskBatchArgs) if native else "vbd_task_batch*")
            else:
                types.append(ctypes.c_void_p if "*" in a else _C_TYPES[a.replace("const ", "").split()[0]])
        out[name] = (_C_TYPES[ret], types)
    return out


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()
    from vilbert import _native
    return _native


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(GOLDEN))


# ---- header, mirror, library ---------------------------------------------------------------------------------------------------
def test_header_declares_the_task_input_entry_points_and_leaves_the_other_headers_alone():
    assert sorted(_prototypes()) == ["vbd_dense_target", "vbd_task_finish_batch"]
    for name in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert ("vbd_" in text) == (name == "vilbert_hip_task_inputs.h"), name
    own = open(HEADER).read()
    assert not any(p in own for p in ("vbx_", "vbo_", "vbt_", "vbp_", "vbh_", "vbf_", "vbl_", "vbi_"))   # (prefixes other tests pin)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\btask_batch\.hip\b", make, flags=re.M)
    assert re.search(r"^HDRS = .*\btask_rows\.h\b.*vilbert_hip_task_inputs\.h\b", make, flags=re.M)
    assert "-ffast-math" not in make and "-ffp-contract=fast" not in make


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes(native)
    assert sorted(native.TASK_INPUT_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.TASK_INPUT_SIGNATURES[name][0] is res, name
        assert native.TASK_INPUT_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbd_[a-z0-9_]+)", nm))) == sorted(protos)
    lib = native.lib()
    for name in protos:                                         # bound with the mirrored types by lib()
        assert getattr(lib, name).argtypes == native.TASK_INPUT_SIGNATURES[name][1]


def test_argument_struct_matches_its_mirror_field_for_field(native):
    body = re.search(r"typedef struct vbd_task_batch \{(.*?)\} vbd_task_batch;", _header_text(), flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:
            fields.append((decl.split("*")[1].strip(), ctypes.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), _C_TYPES[ctype]) for n in names.split(",")]
    A = native.TaskBatchArgs
    assert fields == [(n, t) for n, t in A._fields_]
    assert ctypes.sizeof(A) == 104 and A.total_rows.offset == 16 and A.feat.offset == 24 and A.out_iou.offset == 96


def _good_args(native, **over):
    a = native.TaskBatchArgs()
    a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.total_rows = 2, 6, 2048, 0.0, 9
    for name in ("feat", "boxes", "offsets", "image_wh", "mean_rows", "ref_box", "out_feat", "out_spatials", "out_mask",
                 "out_iou"):
        setattr(a, name, 64)          # fake non-null addresses: the argument checks come before any launch
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    call = lambda **over: lib.vbd_task_finish_batch(None, ctypes.byref(_good_args(native, **over)))
    assert lib.vbd_task_finish_batch(None, None) == BADARG
    for over in (dict(batch=-1), dict(total_rows=-1), dict(max_regions=0), dict(max_regions=-4), dict(feat_dim=0),
                 dict(feat_dim=-8), dict(iou_floor=-0.5), dict(iou_floor=float("nan")), dict(feat=None), dict(boxes=None),
                 dict(offsets=None), dict(image_wh=None), dict(out_feat=None), dict(out_spatials=None), dict(out_mask=None),
                 dict(ref_box=None), dict(out_iou=None)):
        assert call(**over) == BADARG, over
    for over in (dict(feat_dim=2050), dict(feat_dim=6), dict(feat=68), dict(out_feat=72)):
        assert call(**over) == ALIGN, over
    # a byte offset beyond int64: 4 * total_rows * feat_dim, 4 * batch * max_regions * feat_dim
    assert call(batch=0, total_rows=2 ** 62) == RANGE and call(batch=0, total_rows=2 ** 50) == RANGE
    assert call(batch=2 ** 31 - 1, max_regions=2 ** 31 - 1) == RANGE and call(batch=2 ** 20, max_regions=2 ** 30) == RANGE
    # nothing to do: no launch (the optional pointers may both be absent); the checks still come first
    assert call(batch=0) == 0 and call(batch=0, mean_rows=None, ref_box=None, out_iou=None) == 0
    assert call(batch=0, total_rows=0) == 0 and call(batch=0, iou_floor=0.5) == 0
    assert call(batch=0, max_regions=0) == BADARG and call(batch=0, feat_dim=6) == ALIGN and call(batch=0, ref_box=None) == BADARG

    a, b = ctypes.c_void_p(64), ctypes.c_void_p(4096)
    dt = lib.vbd_dense_target
    assert dt(None, 0, 3129, 10, a, a, b, 3129) == 0 and dt(None, 0, 1, 1, a, a, b, 1) == 0
    for args in ((None, -1, 7, 2, a, a, b, 7), (None, 4, 0, 2, a, a, b, 7), (None, 4, -7, 2, a, a, b, 7), (None, 4, 7, 0, a, a, b, 7),
                 (None, 4, 7, 2, a, a, b, 6), (None, 4, 7, 2, None, a, b, 7), (None, 4, 7, 2, a, None, b, 7),
                 (None, 4, 7, 2, a, a, None, 7), (None, 0, 7, 2, a, a, b, 6)):
        assert dt(*args) == BADARG, args
    assert dt(None, 2 ** 62, 7, 2, a, a, b, 7) == RANGE and dt(None, 2 ** 58, 7, 2, a, a, b, 8) == RANGE
    assert dt(None, 2 ** 40, 7, 2 ** 22, a, a, b, 7) == RANGE                   # 4 * rows * K


# ---- the restatement against the reference's own datasets ----------------------------------------------------------------------
def golden_sample(g, image_id, tag="img"):
    j = list(g[tag + "_ids"]).index(image_id)
    off = np.concatenate([[0], np.cumsum(g[tag + "_rows"])])
    return dict(feat=g[tag + "_feat"][off[j]:off[j + 1]], boxes=g[tag + "_boxes"][off[j]:off[j + 1]],
                image_w=int(g[tag + "_wh"][j, 0]), image_h=int(g[tag + "_wh"][j, 1]))


def golden_refer_batch(g, split):
    """(packed batch, ref_box [B, 4] fp32, iou floor, expected outputs) of a refer-expression split of the golden file: the
    training split appends the ground-truth rows (which do not enter the mean) and floors the IoU at 0.5."""
    from vilbert import task_pipeline as tp
    pre = "refer_%s_" % split
    samples, mean_rows = [], []
    for image_id in g[pre + "image"]:
        s = golden_sample(g, image_id)
        mean_rows.append(len(s["feat"]))
        if split == "train":
            gt = golden_sample(g, image_id, "gt")
            s = dict(s, feat=np.concatenate([s["feat"], gt["feat"]]), boxes=np.concatenate([s["boxes"], gt["boxes"]]))
        samples.append(s)
    x = g[pre + "ref_xywh"]                # float64, as the annotation holds it; the dataset adds in double, then .float()
    ref_box = np.stack([x[:, 0], x[:, 1], x[:, 0] + x[:, 2], x[:, 1] + x[:, 3]], axis=1).astype(np.float32)
    want = tuple(g[pre + n] for n in ("features", "spatials", "image_mask", "target"))
    return tp.pack_task_samples(samples, mean_rows=mean_rows), ref_box, 0.5 if split == "train" else 0.0, want


def same_bits(got, want, name):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if got.dtype == np.float32:
        got, want = got.view(np.int32), want.view(np.int32)
    assert np.array_equal(got, want), name


def test_golden_covers_the_cases_it_is_there_for(golden):
    g = golden
    R = int(g["max_regions"])
    kept = g["vqa_image_mask"].sum(1)
    assert g["img_feat"].shape[1] == 2048 and 4 <= len(g["img_ids"]) <= 6
    assert (kept < R).any() and (g["img_rows"] + 1 == R).any() and (g["img_rows"] + 1 > R).any()
    assert (g["img_wh"].astype(np.int64).prod(1) > 2 ** 24).any()
    assert (g["refer_train_image_mask"].sum(1) > 1 + np.array([golden_sample(g, i)["feat"].shape[0]
                                                              for i in g["refer_train_image"]])).any()     # a kept GT row
    assert (g["refer_train_target"] == 1).any() and (g["refer_val_target"] > 0).sum() >= 4
    assert ((g["refer_val_target"] > 0) & (g["refer_val_target"] < 0.5)).any()
    assert os.path.getsize(GOLDEN) < 500 * 1024


def test_restatement_equals_the_reference_reader_exactly(golden):
    g = golden
    s = golden_sample(g, int(g["img_ids"][0]))
    n = s["feat"].shape[0]
    from vilbert import task_pipeline as tp
    feat, spatials, mask = tr.finish_task_batch(tp.pack_task_samples([s]), n + 1)
    assert int(g["reader_num_boxes"]) == n + 1 and mask.tolist() == [[1] * (n + 1)]
    same_bits(feat[0], g["reader_features"], "reader features")
    assert g["reader_boxes"].dtype == np.float64                       # (an int row on top of fp32 rows)
    same_bits(spatials[0], g["reader_boxes"].astype(np.float32), "reader boxes")
    assert np.array_equal(spatials[0].astype(np.float64), g["reader_boxes"])


def test_restatement_equals_the_reference_vqa_dataset_exactly(golden):
    from vilbert import task_pipeline as tp
    g = golden
    packed = tp.pack_task_samples([golden_sample(g, i) for i in g["vqa_image"]])
    got = tr.finish_task_batch(packed, int(g["max_regions"]))
    for a, name in zip(got, ("vqa_features", "vqa_spatials", "vqa_image_mask")):
        same_bits(a, g[name], name)
    same_bits(tr.dense_target(g["vqa_labels"], g["vqa_scores"], int(g["num_labels"])), g["vqa_target"], "vqa_target")
    assert not g["vqa_co_attention_mask"].any() and g["vqa_co_attention_mask"].dtype == np.float32


@pytest.mark.parametrize("split", ["val", "train"])
def test_restatement_equals_the_reference_refer_dataset_exactly(golden, split):
    packed, ref_box, floor, want = golden_refer_batch(golden, split)
    got = tr.finish_task_batch(packed, int(golden["max_regions"]), ref_box=ref_box, iou_floor=floor)
    for a, b, name in zip(got, want, ("features", "spatials", "image_mask", "target")):
        same_bits(a, b, "%s %s" % (split, name))


@pytest.mark.parametrize("n", [1, 2, 7, 36, 100])
def test_restatement_mean_is_numpys_sum_over_rows_divided_by_the_count(n):
    """Full-mantissa data of mixed magnitude: any other order of the additions, a pairwise sum or a double accumulator would
    show in the last bits of some of the 2048 columns."""
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n, 2048)) * np.exp(rng.uniform(-4, 4, (n, 1)))).astype(np.float32)
    assert x.flags["C_CONTIGUOUS"]
    want = np.sum(x, axis=0) / n                                       # the reader's line, n a Python int
    assert want.dtype == np.float32
    same_bits(tr.mean_row(x), want, "mean of %d rows" % n)
    if n >= 7:
        assert not np.array_equal(tr.mean_row(x[::-1]), want)          # the order is observable on this data
        assert not np.array_equal((x.astype(np.float64).sum(0) / n).astype(np.float32), want)


def test_restatement_edges():
    p = tr.make_packed([3, 1], 8, seed=1, mean_rows=[2, 1])
    feat, sp, mask, iou = tr.finish_task_batch(p, 1, ref_box=np.zeros((2, 4), np.float32))
    same_bits(feat[0, 0], tr.mean_row(p["feat"][:2]), "mean over the leading rows, R = 1")
    assert mask.tolist() == [[1], [1]] and sp[:, 0].tolist() == [[0, 0, 1, 1, 1]] * 2 and iou.shape == (2, 1, 1)
    # exactly 0.5 survives a floor of 0.5; the next float below does not
    half = tr.iou_px([[0, 0, 0, 1]], [0, 0, 0, 0])
    assert half.tolist() == [0.5]
    assert tr.iou_px([[0, 0, 9, 9]], [0, 0, 9, 9]).tolist() == [1.0]
    assert tr.iou_px([[0, 0, 9, 9]], [20, 20, 30, 30]).tolist() == [0.0]          # disjoint: iw, ih clamp to 0
    assert tr.iou_px([[0, 0, 9, 9]], [10, 0, 19, 9]).tolist() == [0.0]            # one pixel apart: iw = 0 exactly
    assert tr.iou_px([[0, 0, 9, 9]], [9, 0, 18, 9]).tolist() == [np.float32(10) / np.float32(190)]   # touching: one shared column
    # dense target: the last duplicate wins, -1 and out-of-range labels are ignored, the gap keeps its contents
    out = np.full((2, 9), 7.0, np.float32)
    t = tr.dense_target(np.array([[3, 6, 3, -1], [7, -5, 0, 0]], np.int32), np.array([[.1, .2, .3, .4], [.5, .6, .7, .8]], np.float32),
                        7, ldt=9, out=out)
    assert t[0].tolist() == [0, 0, 0, np.float32(.3), 0, 0, np.float32(.2), 7, 7]
    assert t[1].tolist() == [np.float32(.8), 0, 0, 0, 0, 0, 0, 7, 7]


# ---- the packer ----------------------------------------------------------------------------------------------------------------
def test_raw_item_and_pack_round_trip_and_refusals():
    from vilbert import task_pipeline as tp
    import vilbert
    for name in ("raw_item", "pack_task_samples", "finish_task_batch", "dense_target", "TaskBatchPipeline"):
        assert getattr(vilbert, name) is getattr(tp, name)
    rng = np.random.default_rng(0)
    items = [dict(image_id=i, image_w=100 + i, image_h=200 + i, num_boxes=n,
                  features=rng.standard_normal(n * 2048).astype(np.float32), boxes=rng.uniform(0, 99, n * 4).astype(np.float32))
             for i, n in enumerate((3, 1, 5))]
    samples = [tp.raw_item(it) for it in items]
    assert [s["feat"].shape for s in samples] == [(3, 2048), (1, 2048), (5, 2048)] and samples[2]["boxes"].shape == (5, 4)
    p = tp.pack_task_samples(samples)
    assert sorted(p) == sorted(tp.PACKED_FIELDS)
    assert p["offsets"].tolist() == [0, 3, 4, 9] and p["offsets"].dtype == np.int64
    assert p["image_wh"].tolist() == [[100, 200], [101, 201], [102, 202]] and p["image_wh"].dtype == np.int32
    assert p["mean_rows"].tolist() == [3, 1, 5] and p["mean_rows"].dtype == np.int32
    assert p["feat"].dtype == np.float32 and p["feat"].shape == (9, 2048) and p["boxes"].shape == (9, 4)
    for b, it in enumerate(items):                                     # unpacking gives the records back
        lo, hi = p["offsets"][b], p["offsets"][b + 1]
        assert np.array_equal(p["feat"][lo:hi].reshape(-1), it["features"])
        assert np.array_equal(p["boxes"][lo:hi].reshape(-1), it["boxes"])
    assert tp.pack_task_samples(samples, mean_rows=[2, 1, 5])["mean_rows"].tolist() == [2, 1, 5]
    empty = dict(samples[0], feat=np.zeros((0, 2048), np.float32), boxes=np.zeros((0, 4), np.float32))
    for bad in (lambda: tp.pack_task_samples([]), lambda: tp.pack_task_samples([samples[0], empty]),
                lambda: tp.pack_task_samples(samples, mean_rows=[4, 1, 5]), lambda: tp.pack_task_samples(samples, mean_rows=[0, 1, 5]),
                lambda: tp.pack_task_samples(samples, mean_rows=[3, 1]),
                lambda: tp.pack_task_samples([dict(samples[0], boxes=samples[0]["boxes"][:2])]),
                lambda: tp.pack_task_samples([samples[0], dict(samples[1], feat=samples[1]["feat"][:, :1024])]),
                lambda: tp.pack_task_samples([dict(samples[0], image_w=0)])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match="HIP device"):              # no CPU fallback
        import torch
        tp.finish_task_batch({k: torch.from_numpy(v) for k, v in p.items()}, 6)


# ---- the span clamp of task_rows.h ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spans(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    work = str(tmp_path_factory.mktemp("taskrows"))
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, DRIVER]
    exe = os.path.join(work, "task_rows_driver_san")
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe], capture_output=True)
    if san.returncode != 0:          # (a compiler without the sanitizer runtimes: the plain build still checks the spans)
        exe = os.path.join(work, "task_rows_driver")
        subprocess.run(base + ["-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    return {line.split("\t")[0]: tuple(int(v) for v in line.split("\t")[1:]) for line in out.splitlines()}


def test_span_clamp_for_well_formed_and_malformed_offsets(spans):
    want = dict(plain=(10, 15, 15, 16), plain_mean=(10, 15, 12, 16), truncated=(10, 15, 15, 6), exactly_full=(10, 5, 5, 6),
                one_region=(10, 15, 15, 1), empty_sample=(10, 0, 0, 1), negative_start=(0, 5, 5, 6), negative_both=(0, 0, 0, 1),
                decreasing=(30, 0, 0, 1), end_too_large=(90, 10, 10, 11), start_too_large=(100, 0, 0, 1),
                start_at_end=(100, 0, 0, 1), int64_extremes=(0, 100, 100, 101), int64_max_both=(100, 0, 0, 1),
                int64_min_end=(5, 0, 0, 1), mean_above_rows=(10, 15, 15, 16), mean_negative=(10, 15, 0, 16),
                mean_zero=(10, 15, 0, 16), mean_with_clamped_rows=(95, 5, 5, 6), no_rows_at_all=(0, 0, 0, 1),
                negative_total=(0, 0, 0, 1), regions_not_positive=(10, 15, 15, 1))
    assert spans == want
    for start, rows, mean, kept in spans.values():                       # what the kernels rely on
        assert 0 <= start and 0 <= rows and start + rows <= 100 and 0 <= mean <= rows and 1 <= kept <= rows + 1


def test_restatement_span_is_the_headers(spans):
    cases = dict(plain=(10, 25, 100, None, 101), plain_mean=(10, 25, 100, 12, 101), truncated=(10, 25, 100, None, 6),
                 negative_start=(-7, 5, 100, None, 6), decreasing=(30, 20, 100, None, 6), end_too_large=(90, 250, 100, None, 101),
                 start_too_large=(150, 160, 100, None, 101), mean_above_rows=(10, 25, 100, 40, 101),
                 mean_negative=(10, 25, 100, -2, 101), mean_with_clamped_rows=(95, 250, 100, 9, 101),
                 int64_extremes=(-2 ** 63, 2 ** 63 - 1, 100, None, 101), negative_total=(0, 5, -4, None, 6))
    for name, args in cases.items():
        assert tr.span(*args) == spans[name], name
