"""Host side of the device-resident region store (csrc/region_store.hip, store_rows.h; include/vilbert_hip_store.h;
vilbert.region_store): the header, its ctypes mirror and the built library agree, every documented argument error comes back
before any launch and in the documented order, the numpy restatement (tests/region_store_restatement.py) equals the packed
restatement on the gathered samples, the id -> span path of csrc/store_rows.h holds for invalid ids and corrupt store words
(through the stand-alone tests/store_span_driver.cpp, built with the host compiler's sanitizers where it has them), and the
Python layer refuses what it documents. No compute is launched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import region_store_restatement as rr
import task_batch_restatement as tr
from test_gemm_plan import CSRC, TESTS, host_compiler
from test_task_batch import same_bits

ROOT = os.path.dirname(TESTS)
HEADER = os.path.join(ROOT, "include", "vilbert_hip_store.h")
DRIVER = os.path.join(TESTS, "store_span_driver.cpp")
BADARG, ALIGN, RANGE = -1, -2, -3
ENTRY_POINTS = ["vbr_store_finish_batch"]
OTHER_PREFIXES = ("vbw_", "vbd_", "vbi_", "vbx_", "vbo_", "vbt_", "vbp_", "vbh_", "vbf_", "vbl_", "vbb_")

# the store of the GPU tests: one row, both sides of the 8-row load batch, more rows than max_regions
STORE_ROWS = [1, 3, 8, 9, 17, 2, 100, 8]
ID_LISTS = {"permuted": [6, 0, 0, 7, 3, 2, 2, 5], "single": [4], "ascending": list(range(len(STORE_ROWS)))}
STORE_MEANS = [1, 1, 8, 4, 16, 2, 100, 3]                   # values including 1 and the full count

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "int": ctypes.c_int}


def store_samples(feat_dim, dtype=np.float32, seed=11):
    """The images of the test store as raw samples (what ``raw_item`` gives), features of `dtype` (float16: exactly
    representable values, so the widened store is the fp32 store)."""
    p = tr.make_packed(STORE_ROWS, feat_dim, seed=seed)
    feat = p["feat"].astype(np.float16) if np.dtype(dtype) == np.float16 else p["feat"]
    off = p["offsets"]
    return [dict(feat=feat[off[i]:off[i + 1]], boxes=p["boxes"][off[i]:off[i + 1]], image_w=int(p["image_wh"][i, 0]),
                 image_h=int(p["image_wh"][i, 1])) for i in range(len(STORE_ROWS))]


def store_arrays(samples, mean_rows=None):
    """The five arrays of a store holding `samples`, as numpy (the restatement's `store`)."""
    from vilbert import task_pipeline as tp
    p = tp.pack_task_samples(samples, mean_rows=mean_rows, dtype=np.asarray(samples[0]["feat"]).dtype)
    return dict(feat=p["feat"], boxes=p["boxes"], image_offsets=p["offsets"], image_wh=p["image_wh"],
                mean_rows=None if mean_rows is None else p["mean_rows"])


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototypes(native=None):
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            if "vbr_store_batch*" in a:
                types.append(ctypes.POINTER(native.StoreBatchArgs) if native else "vbr_store_batch*")
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


# ---- header, mirror, library ---------------------------------------------------------------------------------------------------
def test_header_declares_exactly_the_store_entry_point_and_names_no_other_headers_prefix():
    assert sorted(_prototypes()) == ENTRY_POINTS
    for name in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert ("vbr_" in text) == (name == "vilbert_hip_store.h"), name
    own = open(HEADER).read()
    for prefix in OTHER_PREFIXES:                                 # the other headers are referred to by file name only
        assert prefix not in own, prefix
    assert "vilbert_hip_task_inputs.h" in own and "vilbert_hip_wire.h" in own
    text = _header_text()
    for name, value in (("VBR_FEAT_F32", 0), ("VBR_FEAT_F16", 1), ("VBR_OUT_F32", 0), ("VBR_OUT_BF16", 1)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bwire16\.hip\b.*\bregion_store\.hip\b", make, flags=re.M)     # after the sources that were there
    assert re.search(r"^HDRS = .*vilbert_hip_wire\.h\b.*\bstore_rows\.h\b.*vilbert_hip_store\.h\b", make, flags=re.M)
    assert re.search(r"^HDRS = .*\btask_meta\.h\b", make, flags=re.M)
    assert "-ffast-math" not in make and "-ffp-contract=fast" not in make


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes(native)
    assert sorted(native.STORE_SIGNATURES) == sorted(protos) == ENTRY_POINTS
    for name, (res, args) in protos.items():
        assert native.STORE_SIGNATURES[name][0] is res, name
        assert native.STORE_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbr_[a-z0-9_]+)", nm))) == ENTRY_POINTS
    assert getattr(native.lib(), ENTRY_POINTS[0]).argtypes == native.STORE_SIGNATURES[ENTRY_POINTS[0]][1]
    assert native.STORE_FEAT_KINDS == {torch.float32: 0, torch.float16: 1}


def test_argument_struct_matches_its_mirror_field_for_field(native):
    body = re.search(r"typedef struct vbr_store_batch \{(.*?)\} vbr_store_batch;", _header_text(), flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:
            fields.append((decl.split("*")[1].strip(), ctypes.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), _C_TYPES[ctype]) for n in names.split(",")]
    A = native.StoreBatchArgs
    assert fields == [(n, t) for n, t in A._fields_] and len(fields) == 19
    stated = re.search(r"\} vbr_store_batch;\s*/\* (\d+) bytes \*/", open(HEADER).read())
    assert stated and int(stated.group(1)) == 128 == ctypes.sizeof(A)
    assert A.feat_kind.offset == 16 and A.total_rows.offset == 24 and A.num_images.offset == 32 and A.feat.offset == 40
    assert A.image_ids.offset == 80 and A.out_iou.offset == 120


def test_resource_file_holds_the_three_store_instantiations_without_scratch(native):
    """The feature kernel of csrc/feat_rows.h once per (store, output) kind - In = f (fp32) or DF16_ (binary16), Out = f or the
    bf16 element - for the store's argument struct, in the resource file of region_store.hip and nowhere else; none spills."""
    csrc = os.path.dirname(native.LIB_PATH)
    text = open(os.path.join(csrc, "region_store.resource.txt")).read()
    found = [(fn, int(s)) for fn, s in re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, flags=re.S)]
    feat = [(fn, s) for fn, s in found if "task_feat_kernel" in fn]
    assert len(feat) == 3, found
    for kind in ("Iff", "IDF16_f", "IDF16_NS_4bf16E"):
        assert [s for fn, s in feat if "task_feat_kernel%s15vbr_store_batch" % kind in fn] == [0], (kind, feat)
    meta = [(fn, s) for fn, s in found if "task_meta_kernel" in fn]
    assert len(meta) == 1 and "vbr_store_batch" in meta[0][0] and meta[0][1] == 0
    assert len(found) == 4                                        # no kernel of its own
    for name in os.listdir(csrc):
        if name.endswith(".resource.txt") and name != "region_store.resource.txt":
            assert "vbr_store_batch" not in open(os.path.join(csrc, name)).read(), name


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def _args(native, **over):
    a = native.StoreBatchArgs()
    a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.feat_kind, a.out_kind, a.total_rows, a.num_images = 2, 6, 2048, 0.0, 1, 0, 9, 3
    for name, _ in a._fields_[8:]:
        setattr(a, name, 64)          # fake non-null 16-byte-aligned addresses: the argument checks come before any launch
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_argument_errors_do_not_need_a_gpu_and_come_in_the_documented_order(native):
    lib = native.lib()
    call = lambda **over: lib.vbr_store_finish_batch(None, ctypes.byref(_args(native, **over)))
    assert lib.vbr_store_finish_batch(None, None) == BADARG
    required = ("feat", "boxes", "image_offsets", "image_wh", "image_ids", "out_feat", "out_spatials", "out_mask")
    for over in ([dict(batch=-1), dict(total_rows=-1), dict(num_images=-1), dict(max_regions=0), dict(max_regions=-4),
                  dict(feat_dim=0), dict(feat_dim=-8), dict(iou_floor=-0.5), dict(iou_floor=float("nan")), dict(feat_kind=2),
                  dict(feat_kind=-1), dict(out_kind=2), dict(out_kind=-1), dict(feat_kind=0, out_kind=1), dict(ref_box=None),
                  dict(out_iou=None)] + [{n: None} for n in required]):
        assert call(**over) == BADARG, over
    # the column group follows the store: 4 fp32 or 8 binary16 columns
    for over in (dict(feat_dim=12), dict(feat_dim=2052), dict(feat_kind=0, feat_dim=6), dict(feat_kind=0, feat_dim=2050),
                 dict(feat=66), dict(feat=72), dict(out_feat=68), dict(out_feat=72)):
        assert call(**over) == ALIGN, over
    # a byte offset beyond int64: total_rows * feat_dim * (2 or 4), 4 * batch * max_regions * feat_dim
    assert call(batch=0, total_rows=2 ** 62) == RANGE and call(batch=0, total_rows=2 ** 52) == RANGE
    assert call(batch=0, total_rows=2 ** 50) == 0                # 2 * 2^50 * 2048 = 2^62: in range for 2-byte elements
    assert call(batch=0, total_rows=2 ** 50, feat_kind=0) == RANGE            # 4 * 2^50 * 2048 = 2^63
    assert call(batch=2 ** 31 - 1, max_regions=2 ** 31 - 1) == RANGE and call(batch=2 ** 20, max_regions=2 ** 30) == RANGE
    # nothing to do: no launch (the optional pointers may be absent); the checks still come first
    assert call(batch=0) == 0 and call(batch=0, mean_rows=None, ref_box=None, out_iou=None) == 0
    assert call(batch=0, total_rows=0, num_images=0, out_kind=1) == 0 and call(batch=0, iou_floor=0.5) == 0
    assert call(batch=0, feat_kind=0, feat_dim=12) == 0 and call(batch=0, num_images=2 ** 40) == 0
    assert call(batch=0, max_regions=0) == BADARG and call(batch=0, feat_dim=12) == ALIGN and call(batch=0, ref_box=None) == BADARG
    # the documented order: VB_E_BADARG before VB_E_ALIGN before VB_E_RANGE
    assert call(out_kind=2, feat_dim=12) == BADARG and call(boxes=None, feat=66) == BADARG
    assert call(ref_box=None, feat_dim=12, total_rows=2 ** 62) == BADARG and call(feat_kind=0, out_kind=1, out_feat=72) == BADARG
    assert call(feat_dim=12, total_rows=2 ** 62) == ALIGN and call(out_feat=72, batch=2 ** 31 - 1, max_regions=2 ** 31 - 1) == ALIGN


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_mean", [False, True], ids=["all_rows", "mean_rows"])
@pytest.mark.parametrize("ids", sorted(ID_LISTS))
def test_restatement_equals_the_packed_restatement_on_the_gathered_samples(ids, with_mean):
    from vilbert import task_pipeline as tp
    samples = store_samples(16)
    means = STORE_MEANS if with_mean else None
    assert all(1 <= m <= n for m, n in zip(STORE_MEANS, STORE_ROWS)) and 1 in STORE_MEANS and STORE_MEANS[6] == STORE_ROWS[6]
    store = store_arrays(samples, means)
    chosen = ID_LISTS[ids]
    rng = np.random.default_rng(len(chosen))
    ref_box = np.concatenate([rng.uniform(0, 100, (len(chosen), 2)), rng.uniform(100, 300, (len(chosen), 2))], 1).astype(np.float32)
    for R in (1, 2, 9, 37):
        packed = tp.pack_task_samples([samples[i] for i in chosen], mean_rows=None if means is None else [means[i] for i in chosen])
        want = tr.finish_task_batch(packed, R, ref_box=ref_box, iou_floor=0.5)
        got = rr.finish_store_batch(store, chosen, R, ref_box=ref_box, iou_floor=0.5)
        for g, w, name in zip(got, want, ("features", "spatials", "image_mask", "target")):
            same_bits(g, w, "%s R=%d" % (name, R))


def test_restatement_invalid_ids_and_the_filled_part():
    samples = store_samples(8)
    store = store_arrays(samples, STORE_MEANS)
    ids = [-1, 3, len(STORE_ROWS), 2 ** 40, 0]
    ref_box = np.tile(np.array([[10, 10, 200, 200]], np.float32), (5, 1))
    got = rr.finish_store_batch(store, ids, 9, ref_box=ref_box)
    want = rr.finish_store_batch(store, [3, 0], 9, ref_box=ref_box[:2])
    for g, w in zip(got, want):
        assert not g[[0, 2, 3]].any()                               # all padding, mask row of zeros
        same_bits(g[[1, 4]], w, "valid neighbours")
    assert got[2][1, 0] == 1 and got[2][4, 0] == 1
    # only the filled part counts: an id at or beyond num_images is invalid, rows at or beyond total_rows are not read
    part = rr.finish_store_batch(store, [1, 2, 3], 20, total_rows=8, num_images=3)
    assert part[2].sum(1).tolist() == [4, 5, 0]
    assert rr.image_span(store, 2, 8, 3, 20) == (4, 4, 4, 5) and rr.image_span(store, 3, 8, 3, 20) == (0, 0, 0, 0)


# ---- the id -> span path of store_rows.h -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spans(tmp_path_factory):
    cxx = host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler: neither c++ on PATH nor ROCm's clang++")
    work = str(tmp_path_factory.mktemp("storespan"))
    base = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I", CSRC, DRIVER]
    exe = os.path.join(work, "store_span_driver_san")
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe], capture_output=True)
    if san.returncode != 0:          # (a compiler without the sanitizer runtimes: the plain build still checks the spans)
        exe = os.path.join(work, "store_span_driver")
        subprocess.run(base + ["-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr                       # the driver's own checks: bounds, reads, the id rule
    return {line.split("\t")[0]: tuple(int(v) for v in line.split("\t")[1:]) for line in run.stdout.splitlines()}


def test_driver_spans_for_valid_invalid_and_corrupt_words(spans):
    """(image, start, rows, mean, kept, offset words read, mean words read) per case."""
    want = dict(first=(0, 0, 3, 3, 4, 2, 0), last=(3, 40, 60, 60, 61, 2, 0), truncated=(2, 4, 36, 36, 6, 2, 0),
                one_region=(2, 4, 36, 36, 1, 2, 0), with_mean=(2, 4, 36, 36, 37, 2, 1), mean_when_truncated=(3, 40, 60, 9, 4, 2, 1),
                decreasing=(1, 30, 0, 0, 1, 2, 0), offset_past_total=(1, 90, 10, 10, 11, 2, 0), start_past_total=(2, 100, 0, 0, 1, 2, 0),
                negative_offset=(0, 0, 5, 5, 6, 2, 0), int64_extremes=(0, 0, 100, 100, 101, 2, 0), int64_max_both=(0, 100, 0, 0, 1, 2, 0),
                mean_above_rows=(1, 3, 1, 1, 2, 2, 1), mean_negative=(1, 3, 1, 0, 2, 2, 1), filled_part_only=(2, 4, 36, 36, 37, 2, 0),
                negative_total=(1, 0, 0, 0, 1, 2, 0), regions_not_positive=(2, 4, 36, 36, 1, 2, 0))
    invalid = ("id_minus_one", "id_num_images", "id_past_num_images", "id_2_to_40", "id_int64_max", "id_int64_min",
               "id_minus_one_as_u32", "empty_store", "empty_store_negative")
    want.update({name: (-1, 0, 0, 0, 0, 0, 0) for name in invalid})            # nothing read, nothing owned
    assert spans == want


def test_restatement_span_is_the_headers(spans):
    good = dict(image_offsets=np.array([0, 3, 4, 40, 100]), mean_rows=None)
    means = dict(good, mean_rows=np.array([2, 1, 36, 9]))
    cases = dict(first=(good, 0, 100, 101), last=(good, 3, 100, 101), truncated=(good, 2, 100, 6), with_mean=(means, 2, 100, 101),
                 mean_when_truncated=(means, 3, 100, 4), id_minus_one=(means, -1, 100, 101), id_num_images=(means, 4, 100, 101),
                 id_2_to_40=(means, 2 ** 40, 100, 101), filled_part_only=(good, 2, 40, 101),
                 decreasing=(dict(image_offsets=np.array([0, 30, 20, 100])), 1, 100, 101),
                 offset_past_total=(dict(image_offsets=np.array([0, 90, 250, 300])), 1, 100, 101))
    for name, (store, i, total, R) in cases.items():
        assert rr.image_span(store, i, total, len(store["image_offsets"]) - 1, R) == spans[name][1:5], name


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_python_side_refusals_come_before_any_device_work():
    import vilbert
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    assert vilbert.RegionStore is rs.RegionStore and vilbert.StoreBatchPipeline is rs.StoreBatchPipeline
    with pytest.raises(RuntimeError, match="HIP device"):                       # no CPU fallback
        rs.RegionStore("cpu", 10, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        rs.RegionStore.from_samples(store_samples(8, np.float16), "cpu")
    for bad in (dict(dtype=torch.bfloat16), dict(feat_dim=12), dict(feat_dim=4), dict(feat_dim=0)):
        with pytest.raises(ValueError):
            rs.RegionStore("cuda:0", 10, 2, **bad)
    assert rs.RegionStore("cuda:0", 10, 2, feat_dim=4, dtype=torch.float32).nbytes == 10 * 4 * 4 + 10 * 16 + 3 * 8 + 2 * 8 + 2 * 4
    half, wide = store_samples(8, np.float16), store_samples(8)
    store = rs.RegionStore("cuda:0", 3, 2, feat_dim=8)                          # the constructor touches no device
    assert (store.num_images, store.total_rows, store.dtype, store.nbytes) == (0, 0, torch.float16, 3 * 8 * 2 + 3 * 16 + 24 + 16 + 8)
    # dtype mismatches: nothing is narrowed, nothing is widened
    with pytest.raises(ValueError, match="never narrows or widens"):
        store.add(tp.pack_task_samples(wide[:1]))
    with pytest.raises(ValueError, match="never narrows or widens"):
        rs.RegionStore("cuda:0", 3, 2, feat_dim=8, dtype=torch.float32).add(tp.pack_task_samples(half[:1], dtype=np.float16))
    with pytest.raises(ValueError, match="width"):
        store.add(tp.pack_task_samples(store_samples(16, np.float16)[:1], dtype=np.float16))
    with pytest.raises(ValueError, match="with_mean_rows"):
        store.add(tp.pack_task_samples(half[1:2], mean_rows=[2], dtype=np.float16))
    # past either capacity: refused whole, the counts stay
    for chunk in (half[:3], half[1:3], half[2:3]):                              # 3 images; 2 images of 11 rows; 1 image of 8 rows
        with pytest.raises(ValueError, match="capacity"):
            store.add(tp.pack_task_samples(chunk, dtype=np.float16))
        assert (store.num_images, store.total_rows) == (0, 0) and store.feat is None
    # host ids: integers in [0, num_images)
    for ids in ([0], [-1], np.array([0.0]), np.array([[0]]), [2 ** 40]):
        with pytest.raises(ValueError, match="image_ids"):
            store.batch(ids, 4)
    store.num_images = 5                                                        # (as if filled: the id check is host arithmetic)
    assert store.host_ids([4, 0, 0]).tolist() == [4, 0, 0] and store.host_ids(np.array([3], np.int32)).dtype == np.int64
    assert store.host_ids([]).shape == (0,)
    for ids in ([5], [0, -1], [1.5]):
        with pytest.raises(ValueError, match="image_ids"):
            store.host_ids(ids)
    with pytest.raises(ValueError, match="float16 features"):                   # bf16 output only from a float16 store
        rs.RegionStore("cuda:0", 3, 2, feat_dim=8, dtype=torch.float32).batch([], 4, out_dtype=torch.bfloat16)


def test_pipeline_keyword_refusals_and_fields():
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    from vilbert.staging import StagedPipeline
    half = rs.RegionStore("cuda:0", 3, 2, feat_dim=8)
    wide = rs.RegionStore("cuda:0", 3, 2, feat_dim=8, dtype=torch.float32)
    assert issubclass(rs.StoreBatchPipeline, StagedPipeline) and rs.StoreBatchPipeline.wire_fields == ()
    p = rs.StoreBatchPipeline([], half, 6, target=("dense", 7), feature_dtype=torch.bfloat16)
    assert p.wire_dtype == torch.float16 and p.feature_dtype == torch.bfloat16 and p.store is half
    assert p.fields == ("image_ids", "question", "input_mask", "segment_ids", "question_id", "labels", "scores")
    assert not set(tp.PACKED_FIELDS) & set(p.fields) and p.dtypes["image_ids"] == torch.int64
    assert rs.StoreBatchPipeline([], wide, 6).fields[-1] == "target" and rs.StoreBatchPipeline([], wide, 6).wire_dtype is None
    assert rs.StoreBatchPipeline([], wide, 6, target=("iou", 0.5)).fields[-1] == "ref_box"
    with pytest.raises(ValueError, match="float16 features"):
        rs.StoreBatchPipeline([], wide, 6, feature_dtype=torch.bfloat16)
    with pytest.raises(ValueError):
        rs.StoreBatchPipeline([], half, 6, target=("sparse", 3))
    half.num_images = 2
    src = [dict(image_ids=np.array([0, 2]), question=np.zeros((2, 3), np.int64))]
    with pytest.raises(ValueError, match="image_ids"):                         # refused before the pipeline touches a device
        next(iter(rs.StoreBatchPipeline(src, half, 6)))
