"""Host side of the half-width (float16) feature wire (csrc/batch.hip, task_batch.hip, wire16.hip; include/vilbert_hip_wire.h; vilbert.input_pipeline and
vilbert.task_pipeline with wire_dtype=torch.float16): the header, its ctypes mirror and the built library agree, argument errors
come back before any launch, the Python layer refuses to narrow fp32 arrays, and the masking case that
tests/test_wire16_gpu.py runs for the fused row clearing is not an empty one. No compute is launched."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import wire16_cases as wc
from test_gemm_plan import CSRC, TESTS

ROOT = os.path.dirname(TESTS)
HEADER = os.path.join(ROOT, "include", "vilbert_hip_wire.h")
BADARG, ALIGN, RANGE = -1, -2, -3
ENTRY_POINTS = ["vbw_concap_finish_batch", "vbw_task_finish_batch", "vbw_widen_f16"]
STRUCTS = {"vbw_concap_batch": ("WireConcapBatch", 128), "vbw_task_batch": ("WireTaskBatch", 112)}

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototypes(native=None):
    """name -> (return ctype, [argument ctypes]) parsed from the header text; a pointer is a plain address, except the pointers
    to the argument structs, which the mirror types."""
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbw_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            struct = [s for s in STRUCTS if s + "*" in a]
            if struct:
                types.append(ctypes.POINTER(getattr(native, STRUCTS[struct[0]][0])) if native else struct[0] + "*")
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
def test_header_declares_the_wire_entry_points_and_names_no_other_headers_entry_point():
    assert sorted(_prototypes()) == ENTRY_POINTS
    for name in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert ("vbw_" in text) == (name == "vilbert_hip_wire.h"), name
    own = open(HEADER).read()
    for prefix in ("vbx_", "vbo_", "vbt_", "vbp_", "vbh_", "vbf_", "vbl_", "vbi_", "vbd_", "vbb_"):     # (other tests pin these)
        assert prefix not in own, prefix
    assert not re.search(r"\bvb_[a-z]", own)                      # the other headers are referred to by file name only
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS = .*\bwire16\.hip\b", make, flags=re.M)
    assert re.search(r"^HDRS = .*\bfeat_rows\.h\b.*vilbert_hip_wire\.h\b", make, flags=re.M)
    gone = "batch_" + "meta"                                      # the header the entry points used to share launches through
    assert gone not in make and not os.path.exists(os.path.join(CSRC, gone + ".h"))


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes(native)
    assert sorted(native.WIRE_SIGNATURES) == sorted(protos) == ENTRY_POINTS
    for name, (res, args) in protos.items():
        assert native.WIRE_SIGNATURES[name][0] is res, name
        assert native.WIRE_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbw_[a-z0-9_]+)", nm))) == ENTRY_POINTS
    lib = native.lib()
    for name in protos:                                         # bound with the mirrored types by lib()
        assert getattr(lib, name).argtypes == native.WIRE_SIGNATURES[name][1]
    assert native.WIRE_OUT_KINDS == {torch.float32: 0, torch.bfloat16: 1}
    assert re.search(r"#define VBW_OUT_F32 0\b", _header_text()) and re.search(r"#define VBW_OUT_BF16 1\b", _header_text())


@pytest.mark.parametrize("struct", sorted(STRUCTS))
def test_argument_structs_match_their_mirrors_field_for_field(native, struct):
    mirror, size = STRUCTS[struct]
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header_text(), flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:
            fields.append((decl.split("*")[1].strip(), ctypes.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), _C_TYPES[ctype]) for n in names.split(",")]
    A = getattr(native, mirror)
    assert fields == [(n, t) for n, t in A._fields_]
    # the size the header states next to the closing brace
    stated = re.search(r"\} %s;\s*/\* (\d+) bytes \*/" % struct, open(HEADER).read())
    assert stated and int(stated.group(1)) == size == ctypes.sizeof(A)
    if struct == "vbw_concap_batch":
        assert A.image_feat.offset == 24 and A.zero_row.offset == 80 and A.out_lm_label_ids.offset == 120
    else:
        assert A.iou_floor.offset == 16 and A.total_rows.offset == 24 and A.feat.offset == 32 and A.out_iou.offset == 104


def test_resource_file_of_the_new_source_shows_no_scratch(native):
    """Every feature kernel by its mangled name, in the resource file of the source that launches it: the instantiations of
    csrc/feat_rows.h - In = f (fp32) or DF16_ (binary16), Out = f or the bf16 element - batch.hip's own fp32 kernel (no
    template arguments: ...kernelE) and the flat widening kernel. Each is there exactly once and none spills."""
    scratch = {}
    for src in ("batch", "task_batch", "wire16"):
        text = open(os.path.join(os.path.dirname(native.LIB_PATH), src + ".resource.txt")).read()
        found = re.findall(r"Function Name: (\S+).*?ScratchSize \[bytes/lane\]: (\d+)", text, flags=re.S)
        scratch[src] = [(fn, int(s)) for fn, s in found if "feat_kernel" in fn or "widen" in fn]
    for src, kernel, kinds in (("batch", "concap_feat_kernel", ("Eii", "IDF16_f", "IDF16_NS_4bf16E")),
                               ("task_batch", "task_feat_kernel", ("Iff", "IDF16_f", "IDF16_NS_4bf16E"))):
        assert len(scratch[src]) == 3, scratch[src]
        for kind in kinds:
            assert [s for fn, s in scratch[src] if kernel + kind in fn] == [0], (kernel, kind, scratch[src])
    assert len(scratch["wire16"]) == 1 and "widen_f16_kernel" in scratch["wire16"][0][0] and scratch["wire16"][0][1] == 0


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def _concap_args(native, **over):
    a = native.WireConcapBatch()
    a.batch, a.regions, a.tokens, a.feat_dim, a.objective, a.out_kind = 2, 5, 6, 2048, 0, 0
    for name, _ in a._fields_[6:]:
        setattr(a, name, 64)          # fake non-null 16-byte-aligned addresses: the argument checks come before any launch
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _task_args(native, **over):
    a = native.WireTaskBatch()
    a.batch, a.max_regions, a.feat_dim, a.out_kind, a.iou_floor, a.total_rows = 2, 6, 2048, 0, 0.0, 9
    for name, _ in a._fields_[6:]:
        setattr(a, name, 64)
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_concap_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    call = lambda **over: lib.vbw_concap_finish_batch(None, ctypes.byref(_concap_args(native, **over)))
    assert lib.vbw_concap_finish_batch(None, None) == BADARG
    pointers = [n for n, _ in native.WireConcapBatch._fields_[6:] if n != "zero_row"]
    assert len(pointers) == 12
    for over in ([dict(batch=-1), dict(regions=0), dict(regions=-3), dict(tokens=0), dict(tokens=-1), dict(feat_dim=0),
                  dict(feat_dim=-8), dict(out_kind=2), dict(out_kind=-1)] + [{n: None} for n in pointers]):
        assert call(**over) == BADARG, over
    for over in (dict(feat_dim=12), dict(feat_dim=2052), dict(image_feat=66), dict(image_feat=72), dict(out_image_feat=68),
                 dict(out_image_feat=72)):
        assert call(**over) == ALIGN, over
    # a byte offset beyond int64: 2 * batch * regions * feat_dim, 4 * batch * (regions + 1) * feat_dim
    big = 2 ** 31 - 1
    assert call(batch=big, regions=big, feat_dim=big - 7) == RANGE and call(batch=2 ** 21, regions=2 ** 20, feat_dim=2 ** 20) == RANGE
    # nothing to do: no launch; the checks still come first; zero_row is optional
    assert call(batch=0) == 0 and call(batch=0, zero_row=None) == 0 and call(batch=0, out_kind=1) == 0
    assert call(batch=0, feat_dim=12) == ALIGN and call(batch=0, out_kind=2) == BADARG and call(batch=0, image_loc=None) == BADARG


def test_task_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    call = lambda **over: lib.vbw_task_finish_batch(None, ctypes.byref(_task_args(native, **over)))
    assert lib.vbw_task_finish_batch(None, None) == BADARG
    for over in (dict(batch=-1), dict(total_rows=-1), dict(max_regions=0), dict(max_regions=-4), dict(feat_dim=0),
                 dict(feat_dim=-8), dict(iou_floor=-0.5), dict(iou_floor=float("nan")), dict(out_kind=2), dict(out_kind=-1),
                 dict(feat=None), dict(boxes=None), dict(offsets=None), dict(image_wh=None), dict(out_feat=None),
                 dict(out_spatials=None), dict(out_mask=None), dict(ref_box=None), dict(out_iou=None)):
        assert call(**over) == BADARG, over
    for over in (dict(feat_dim=12), dict(feat_dim=2052), dict(feat=66), dict(feat=72), dict(out_feat=72)):
        assert call(**over) == ALIGN, over
    # a byte offset beyond int64: 2 * total_rows * feat_dim (the 2-byte input), 4 * batch * max_regions * feat_dim
    assert call(batch=0, total_rows=2 ** 62) == RANGE and call(batch=0, total_rows=2 ** 52) == RANGE
    assert call(batch=0, total_rows=2 ** 50) == 0                # 2 * 2^50 * 2048 = 2^62: in range for 2-byte elements
    assert call(batch=2 ** 31 - 1, max_regions=2 ** 31 - 1) == RANGE and call(batch=2 ** 20, max_regions=2 ** 30) == RANGE
    assert call(batch=0) == 0 and call(batch=0, mean_rows=None, ref_box=None, out_iou=None) == 0
    assert call(batch=0, total_rows=0, out_kind=1) == 0 and call(batch=0, iou_floor=0.5) == 0
    assert call(batch=0, max_regions=0) == BADARG and call(batch=0, feat_dim=12) == ALIGN and call(batch=0, ref_box=None) == BADARG


def test_widen_argument_errors_do_not_need_a_gpu(native):
    w = native.lib().vbw_widen_f16
    a = ctypes.c_void_p(64)
    assert w(None, 0, a, a) == 0
    assert w(None, -1, a, a) == BADARG and w(None, 8, None, a) == BADARG and w(None, 8, a, None) == BADARG
    assert w(None, 0, None, a) == BADARG
    assert w(None, 8, ctypes.c_void_p(66), a) == ALIGN and w(None, 8, a, ctypes.c_void_p(68)) == ALIGN
    assert w(None, 2 ** 62, a, a) == RANGE


# ---- the Python layer never narrows ----------------------------------------------------------------------------------------------
def _concap_source(feat_dtype, target_dtype):
    from oracle import batch_oracle as bo
    raw = bo.make_raw_batch(3, tokens=6, regions=5, feat_dim=8, n_classes=9, vocab=99, seed=5)
    raw["image_feat"] = raw["image_feat"].astype(feat_dtype)
    raw["image_target"] = raw["image_target"].astype(target_dtype)
    return [tuple(raw[n] for n in bo.RAW_FIELDS)]


@pytest.mark.parametrize("dtypes", [(np.float32, np.float16), (np.float16, np.float32), (np.float32, np.float32),
                                    (np.float64, np.float16)], ids=lambda d: "%s-%s" % (d[0].__name__, d[1].__name__))
def test_pretraining_pipeline_with_a_float16_wire_refuses_other_arrays(dtypes):
    """The refusal comes before the pipeline touches a device: the constructor and the dtype check need none."""
    from vilbert import input_pipeline as ip
    pipe = ip.DeviceBatchPipeline(_concap_source(*dtypes), "cuda:0", wire_dtype=torch.float16)
    assert pipe.wire_dtype == torch.float16 and pipe.feature_dtype == torch.float32
    with pytest.raises(ValueError, match="never narrows"):
        next(iter(pipe))


def test_pipeline_keyword_refusals():
    from vilbert import input_pipeline as ip
    from vilbert import task_pipeline as tp
    for make in (lambda **kw: ip.DeviceBatchPipeline([], "cuda:0", **kw), lambda **kw: tp.TaskBatchPipeline([], "cuda:0", 6, **kw)):
        default = make()
        assert default.wire_dtype is None and default.feature_dtype == torch.float32
        assert make(wire_dtype=torch.float16, feature_dtype=torch.bfloat16).feature_dtype == torch.bfloat16
        with pytest.raises(ValueError, match="float16 features"):          # bf16 output only from the float16 wire
            make(feature_dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="wire_dtype"):
            make(wire_dtype=torch.bfloat16)
        with pytest.raises(ValueError, match="out_dtype"):
            make(wire_dtype=torch.float16, feature_dtype=torch.float16)
    # the functions state the same rule for fp32 features (refused before any device work)
    with pytest.raises(ValueError, match="float16 features"):
        ip.finish_batch(dict(image_feat=torch.zeros(1, 2, 8), lm_label_ids=torch.zeros(1, 3, dtype=torch.int64),
                             image_target=torch.zeros(1, 2, 3)), out_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="float16 features"):
        tp.finish_task_batch(dict(feat=torch.zeros(2, 8), offsets=torch.zeros(2, dtype=torch.int64)), 4, out_dtype=torch.bfloat16)


def test_packer_with_a_float16_dtype_refuses_fp32_features_and_packs_float16_as_it_is():
    from vilbert import task_pipeline as tp
    h = [dict(feat=wc.f16_values((n, 8), n), boxes=np.zeros((n, 4), np.float32), image_w=10, image_h=20) for n in (3, 1)]
    p = tp.pack_task_samples(h, dtype=np.float16)
    assert p["feat"].dtype == np.float16 and p["feat"].shape == (4, 8) and p["offsets"].tolist() == [0, 3, 4]
    assert np.array_equal(p["feat"].view(np.uint16), np.concatenate([s["feat"] for s in h]).view(np.uint16))
    assert p["boxes"].dtype == np.float32 and p["mean_rows"].tolist() == [3, 1]
    wide = [dict(s, feat=wc.widen(s["feat"])) for s in h]
    for bad in (lambda: tp.pack_task_samples(wide, dtype=np.float16), lambda: tp.pack_task_samples([h[0], wide[1]], dtype=np.float16),
                lambda: tp.pack_task_samples(h, dtype=np.float64)):
        with pytest.raises(ValueError):
            bad()
    # the default keeps today's host-side widening of a float16 sample
    d = tp.pack_task_samples(h)
    assert d["feat"].dtype == np.float32 and np.array_equal(d["feat"], wc.widen(p["feat"]))
    src = [dict(tp.pack_task_samples(wide), question=np.zeros((2, 3), np.int64))]
    with pytest.raises(ValueError, match="never narrows"):
        next(iter(tp.TaskBatchPipeline(src, "cuda:0", 6, wire_dtype=torch.float16)))


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------
def test_float16_test_values_cover_the_special_cases():
    x = wc.f16_values((3, 5, 8), 0)
    bits = x.view(np.uint16).ravel()
    assert x.dtype == np.float16 and np.isfinite(x).all()
    assert (bits == 0x0000).any() and (bits == 0x8000).any() and (bits == 0x7BFF).any() and float(x.max()) == 65504.0
    sub = (bits & 0x7C00) == 0
    assert (sub & ((bits & 0x03FF) != 0)).sum() >= 4                       # subnormals
    assert len(np.unique(bits & 0x03FF)) > 60                             # full mantissas
    assert np.array_equal(wc.widen(x).astype(np.float16).view(np.uint16).ravel(), bits)      # widening is exact


def test_masking_case_of_the_gpu_test_flags_some_valid_regions_and_not_others():
    """tests/test_wire16_gpu.py runs MASK_CASE through the fused row clearing: at least one valid region is flagged (a row that
    must come out as zeros and stay out of the mean) and at least one is not, in one sample."""
    raw, feat = wc.mask_case_raw()
    c = wc.MASK_CASE
    assert feat.shape == (c["B"], c["R"], c["F"]) == (4, 7, 16) and raw["input_ids"].shape == (4, 9) and c["p"] == 0.5
    flags = wc.mask_case_flags(raw)
    valid = raw["image_mask"] != 0
    assert flags.shape == valid.shape and flags.dtype == np.uint8
    assert (flags[valid] != 0).any() and (flags[valid] == 0).any()
    assert any((flags[b][valid[b]] != 0).any() and (flags[b][valid[b]] == 0).any() for b in range(c["B"]))
    assert not flags[~valid].any()
    assert np.abs(feat[flags != 0].astype(np.float32)).sum() > 0            # clearing them changes something
