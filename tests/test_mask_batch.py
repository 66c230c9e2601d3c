"""Host side of the device-side MLM and region masking (csrc/mask_batch.hip; vilbert.input_pipeline.mask_batch, Masking,
unmasked_preprocess): the header include/vilbert_hip_inputs.h, its ctypes mirror and the built library agree, argument errors
come back without a GPU, and the numpy restatement (tests/masking_restatement.py) - the thing the kernels are held to bit for bit
in tests/test_mask_batch_gpu.py - has the statistics of the reference's rule. No compute is launched here.

Bands: a count of k successes out of n sites with probability q may deviate from n q by 4 sqrt(n q (1 - q)) (4 binomial standard
deviations; a fair generator leaves such a band once in ~16,000 draws). The seeds below are fixed, so each check is deterministic;
this file is where it is confirmed that those seeds keep the restatement alone inside the bands."""
import ast
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import masking_restatement as mr
from dropout_restatement import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vilbert-multi-task_amd")
HEADER = os.path.join(ROOT, "include", "vilbert_hip_inputs.h")
VOCAB, MASK_ID, P = 30522, 103, 0.15
SEEDS = (0x5EED0001, 0x5EED0002, 77)

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "int": ctypes.c_int, "uint64_t": ctypes.c_uint64}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _prototypes(native=None):
    """name -> (return ctype, [argument ctypes]) parsed from the header text; a pointer is a plain address, except the pointer to
    the argument struct, which the mirror types."""
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbi_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header_text()):
        types = []
        for a in args.split(","):
            a = a.strip()
            if "vbi_mask_args*" in a:
                types.append(ctypes.POINTER(native.MaskArgs) if native else "vbi_mask_args*")
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


def within(k, n, q, what):
    sd = np.sqrt(n * q * (1.0 - q))
    print("%s: %d of %d (expected %.1f, 4 sd = %.1f)" % (what, k, n, n * q, 4 * sd))
    return abs(k - n * q) <= 4.0 * sd


# ---- header, mirror, library ---------------------------------------------------------------------------------------------------
def test_header_declares_the_input_entry_points_and_leaves_the_other_headers_alone():
    assert sorted(_prototypes()) == ["vbi_concap_mask_batch", "vbi_zero_rows"]
    for name in os.listdir(os.path.join(ROOT, "include")):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert ("vbi_" in text) == (name == "vilbert_hip_inputs.h"), name
    own = open(HEADER).read()
    assert not any(p in own for p in ("vbx_", "vbo_", "vbt_", "vbp_", "vbh_", "vbf_", "vbl_"))      # (prefixes other tests pin)
    make = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bmask_batch\.hip\b", make, flags=re.M)
    assert re.search(r"^HDRS = .*vilbert_hip_inputs\.h\b", make, flags=re.M)


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes(native)
    assert sorted(native.INPUT_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.INPUT_SIGNATURES[name][0] is res, name
        assert native.INPUT_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbi_[a-z0-9_]+)", nm))) == sorted(protos)
    lib = native.lib()
    assert lib.vb_abi_version() == 18
    for name in protos:                                         # bound with the mirrored types by lib()
        assert getattr(lib, name).argtypes == native.INPUT_SIGNATURES[name][1]


def test_argument_struct_matches_its_mirror_field_for_field(native):
    body = re.search(r"typedef struct vbi_mask_args \{(.*?)\} vbi_mask_args;", _header_text(), flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:
            fields.append((decl.split("*")[1].strip(), ctypes.c_void_p))
        else:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), _C_TYPES[ctype]) for n in names.split(",")]
    assert fields == [(n, t) for n, t in native.MaskArgs._fields_]
    assert ctypes.sizeof(native.MaskArgs) == 104 and native.MaskArgs.seed.offset == 24 and native.MaskArgs.zero_row.offset == 96


def _good_args(native, **over):
    a = native.MaskArgs()
    a.batch, a.tokens, a.regions, a.vocab_size, a.mask_token_id, a.p_select, a.seed = 2, 8, 5, VOCAB, MASK_ID, P, 1
    for name in ("input_ids", "input_mask", "image_mask", "overlaps", "out_input_ids", "lm_label_ids", "image_label",
                 "masked_label", "zero_row"):
        setattr(a, name, 64)          # fake non-null addresses: the argument checks come before any launch
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    call = lambda **over: lib.vbi_concap_mask_batch(None, ctypes.byref(_good_args(native, **over)))
    assert lib.vbi_concap_mask_batch(None, None) == -1
    for over in (dict(batch=-1), dict(tokens=0), dict(regions=0), dict(regions=-3), dict(vocab_size=0), dict(mask_token_id=-1),
                 dict(mask_token_id=VOCAB), dict(p_select=-0.01), dict(p_select=1.5), dict(p_select=float("nan")),
                 dict(input_ids=None), dict(input_mask=None), dict(image_mask=None), dict(overlaps=None), dict(out_input_ids=None),
                 dict(lm_label_ids=None), dict(image_label=None), dict(masked_label=None), dict(zero_row=None)):
        assert call(**over) == -1, over
    assert call(batch=2 ** 31 - 1, regions=2 ** 31 - 1) == -3               # batch * regions * regions leaves int64
    assert call(batch=0) == 0 and call(batch=0, p_select=0.0) == 0          # nothing to do: no launch
    assert call(batch=0, tokens=0) == -1                                    # the checks come first

    a = ctypes.c_void_p(64)
    b = ctypes.c_void_p(4096)
    zr = lib.vbi_zero_rows
    assert zr(None, 0, 8, a, 8, a, None, 0) == 0 and zr(None, 0, 8, a, 8, a, b, 8) == 0
    for args in ((None, -1, 8, a, 8, a, None, 0), (None, 4, 0, a, 8, a, None, 0), (None, 4, 8, a, 4, a, None, 0),
                 (None, 4, 8, None, 8, a, None, 0), (None, 4, 8, a, 8, None, None, 0), (None, 4, 8, a, 8, a, b, 4),
                 (None, 4, 8, a, 8, a, a, 8)):
        assert zr(*args) == -1, args
    for args in ((None, 4, 6, a, 8, a, None, 0), (None, 4, 8, ctypes.c_void_p(68), 8, a, None, 0), (None, 4, 8, a, 10, a, None, 0),
                 (None, 4, 8, a, 8, a, ctypes.c_void_p(4104), 8), (None, 4, 8, a, 8, a, b, 9), (None, 0, 6, a, 8, a, None, 0)):
        assert zr(*args) == -2, args
    assert zr(None, 2 ** 62, 8, a, 8, a, None, 0) == -3 and zr(None, 2 ** 62, 8, a, 8, a, b, 8) == -3
    # the element count fits int64, the byte offset 4 * rows * stride does not
    assert zr(None, 2 ** 58, 8, a, 8, a, None, 0) == -3 and zr(None, 2 ** 58, 8, a, 8, a, b, 8) == -3
    assert zr(None, 2 ** 57, 8, a, 8, a, b, 16) == -3
    assert call(batch=2 ** 20, regions=2 ** 21) == -3                       # 4 * 2^62 bytes of overlaps


# ---- the restatement's statistics ----------------------------------------------------------------------------------------------
def _full_batch(B, T, R, token=5000):
    """Every sample at full length, all ids `token` between [CLS] and [SEP], all boxes real, identity overlaps."""
    ids = np.full((B, T), token, dtype=np.int64)
    ids[:, 0], ids[:, -1] = 101, 102
    ov = np.broadcast_to(np.eye(R, dtype=np.float32), (B, R, R)).copy()
    return ids, np.ones((B, T), np.int64), np.ones((B, R), np.int64), ov


@pytest.mark.parametrize("seed", SEEDS)
def test_selection_rates_and_splits_lie_within_four_standard_deviations(seed):
    B, T, R = 512, 36, 36
    ids, tok_mask, box_mask, ov = _full_batch(B, T, R)
    m = mr.mask_arrays(ids, tok_mask, box_mask, ov, seed, VOCAB, MASK_ID, P)
    lm, out = m["lm_label_ids"], m["input_ids"]
    assert (lm[:, 0] == -1).all() and (lm[:, -1] == -1).all() and (out[:, 0] == 101).all() and (out[:, -1] == 102).all()
    sel = lm != -1
    assert (lm[sel] == 5000).all() and (out[~sel] == ids[~sel]).all()
    k = int(sel.sum())
    assert within(k, B * (T - 2), P, "tokens selected")
    n_mask = int((out[sel] == MASK_ID).sum())
    n_keep = int((out[sel] == 5000).sum())
    n_rand = k - n_mask - n_keep
    assert within(n_mask, k, 0.8, "  -> [MASK]") and within(n_rand, k, 0.1, "  -> random") and within(n_keep, k, 0.1, "  -> kept")
    rand = out[sel][(out[sel] != MASK_ID) & (out[sel] != 5000)]
    assert rand.min() >= 0 and rand.max() < VOCAB and len(np.unique(rand)) > 0.9 * len(rand)
    assert rand.min() < VOCAB // 8 and rand.max() > VOCAB - VOCAB // 8                  # the whole vocabulary is reached

    lab, zero = m["image_label"], m["zero_row"]
    rsel = lab == 1
    assert set(np.unique(lab)) == {-1, 1} and (zero[~rsel] == 0).all()
    kr = int(rsel.sum())
    assert within(kr, B * R, P, "regions selected")
    assert within(int(zero.sum()), kr, 0.9, "  -> zeroed") and within(kr - int(zero.sum()), kr, 0.1, "  -> kept")
    assert np.array_equal(m["masked_label"], rsel.astype(np.int64))                     # identity overlaps: the selection itself


def test_token_and_region_draws_are_independent_streams():
    """T == R and the same positions: the three streams of a sample must not repeat each other."""
    B, T = 64, 36
    L = T
    u = [np.stack([mr.uniform(SEEDS[0], mr.site_index(b, s, L, np.arange(T))) for b in range(B)]) for s in range(3)]
    for s, t in ((0, 1), (0, 2), (1, 2)):
        assert (u[s] == u[t]).mean() < 0.001
        assert abs(np.corrcoef(u[s].ravel(), u[t].ravel())[0, 1]) < 4.0 / np.sqrt(B * T)
    idx = np.concatenate([mr.site_index(b, s, L, np.arange(T)) for b in range(B) for s in range(3)])
    assert len(np.unique(idx)) == 3 * B * T == int(idx.max()) + 1                        # disjoint and dense


def test_two_seeds_differ_and_one_seed_repeats():
    ids, tok_mask, box_mask, ov = _full_batch(16, 36, 36)
    a = mr.mask_arrays(ids, tok_mask, box_mask, ov, 1, VOCAB, MASK_ID, P)
    b = mr.mask_arrays(ids, tok_mask, box_mask, ov, 2, VOCAB, MASK_ID, P)
    again = mr.mask_arrays(ids, tok_mask, box_mask, ov, 1, VOCAB, MASK_ID, P)
    for n in a:
        assert np.array_equal(a[n], again[n]), n
        assert not np.array_equal(a[n], b[n]), n
    agree = ((a["lm_label_ids"] != -1) & (b["lm_label_ids"] != -1)).sum()
    assert agree < 0.5 * (a["lm_label_ids"] != -1).sum()                                 # (p^2 of the sites, not most of them)


def test_batch_seeds_are_a_pure_function_and_never_shifted_copies():
    """Two seeds d apart draw the same uniforms shifted by d / GOLDEN sites (mod 2^64, signed): for every pair of the first 64
    batches that shift lies far outside any index range of a batch (3 * B * L < 2^40 up to a million samples of 300 sites), and the
    selections themselves, compared directly, share no more than chance."""
    from vilbert import input_pipeline as ip
    inv = pow(int(GOLDEN), -1, 1 << 64)
    for seed in (0, 1, SEEDS[0], 2 ** 64 - 1):
        seeds = [ip.batch_seed(seed, i) for i in range(64)]
        assert seeds == [mr.batch_seed(seed, i) for i in range(64)] and seeds == [ip.batch_seed(seed, i) for i in range(64)]
        assert len(set(seeds)) == 64 and seed not in seeds
        for i in range(64):
            for j in range(64):
                if i != j:
                    d = ((seeds[i] - seeds[j]) * inv) % (1 << 64)
                    d = d - (1 << 64) if d >= 1 << 63 else d
                    assert abs(d) > 1 << 40, (seed, i, j, d)
    m = ip.Masking(SEEDS[0], VOCAB, MASK_ID, first_batch=5)
    assert m.batch_seed(3) == ip.batch_seed(SEEDS[0], 8) and (m.p_select, m.vocab_size, m.mask_token_id) == (0.15, VOCAB, MASK_ID)
    # the object counts the batches it hands out: global batch g, whichever iteration it falls into, gets batch_seed(seed, g)
    assert m.next_batch == 5 and [m.next_seed() for _ in range(3)] == [ip.batch_seed(SEEDS[0], g) for g in (5, 6, 7)]
    assert m.next_batch == 8 and m.first_batch == 5 and m.batch_seed(0) == ip.batch_seed(SEEDS[0], 5)
    assert ip.Masking(SEEDS[0], VOCAB, MASK_ID, first_batch=8).next_seed() == m.next_seed()          # a restart at batch 8
    for bad in (dict(p_select=1.5), dict(p_select=-0.1), dict(mask_token_id=VOCAB), dict(vocab_size=0)):
        with pytest.raises(ValueError):
            ip.Masking(**dict(dict(seed=1, vocab_size=VOCAB, mask_token_id=MASK_ID), **bad))
    # direct: the selected-token patterns of batches 0 .. 63 of one run, every pair, at every shift of up to a row
    ids, tok_mask, box_mask, ov = _full_batch(2, 36, 36)
    sel = [mr.mask_arrays(ids, tok_mask, box_mask, ov, ip.batch_seed(7, i), VOCAB, MASK_ID, P)["lm_label_ids"].ravel() != -1
           for i in range(64)]
    for i in range(64):
        for j in range(i + 1, 64):
            for shift in range(0, 36):
                n = len(sel[i]) - shift
                assert not np.array_equal(sel[i][shift:], sel[j][:n]), (i, j, shift)         # j's pattern moved right
                assert not np.array_equal(sel[j][shift:], sel[i][:n]), (i, j, -shift)        # and moved left


def test_edge_samples_of_the_restatement():
    raw = mr.make_unmasked_batch(6, tokens=12, regions=7, feat_dim=8, n_classes=3, vocab=VOCAB, seed=1,
                                 n_tok=[2, 3, 12, 0, 1, 7], n_box=[0, 7, 1, 3, 7, 0])
    all_in = mr.mask_batch(raw, 9, VOCAB, MASK_ID, p_select=1.0)
    none = mr.mask_batch(raw, 9, VOCAB, MASK_ID, p_select=0.0)
    assert (none["lm_label_ids"] == -1).all() and (none["image_label"] == -1).all() and (none["masked_label"] == 0).all()
    assert np.array_equal(none["input_ids"], raw["input_ids"]) and np.array_equal(none["image_feat"], raw["image_feat"])
    assert [(r != -1).sum() for r in all_in["lm_label_ids"]] == [0, 1, 10, 0, 0, 5]      # 1 .. len - 2, nothing for len <= 2
    assert [(r == 1).sum() for r in all_in["image_label"]] == [0, 7, 1, 3, 7, 0]
    assert all_in["image_target"] is raw["image_target"] and (raw["image_label"] == -1).all()
    # an overlap of exactly 0.4 does not mask, the next float does
    ov = np.zeros((1, 3, 3), np.float32)
    ov[0, 0] = [1.0, 0.4, np.nextafter(np.float32(0.4), np.float32(1))]
    m = mr.mask_arrays(np.array([[101, 5, 102]]), np.ones((1, 3), np.int64), np.array([[1, 0, 0]]), ov, 3, VOCAB, MASK_ID, 1.0)
    assert m["image_label"].tolist() == [[1, -1, -1]] and m["masked_label"].tolist() == [[1, 0, 1]]


# ---- unmasked workers ----------------------------------------------------------------------------------------------------------
class _StubPreprocess(object):
    """The two signatures of the reference's BertPreprocessBatch that unmasked_preprocess relies on; this stub masks everything."""

    def __init__(self, tag):
        self.tag = tag

    def random_word(self, tokens, tokenizer, is_next):
        return [0] * len(tokens), list(tokens)

    def random_region(self, image_feat, image_loc, num_boxes, is_next, overlaps):
        return image_feat * 0, image_loc, [1] * num_boxes, np.ones(image_feat.shape[0])

    def other(self):
        return "kept " + self.tag


def test_unmasked_preprocess_selects_nothing_and_hands_the_overlaps_on():
    from vilbert import input_pipeline as ip
    cls = ip.unmasked_preprocess(_StubPreprocess)
    assert issubclass(cls, _StubPreprocess) and cls.__name__ == "Unmasked_StubPreprocess"
    w = cls("x")
    assert w.other() == "kept x"
    tokens = [7, 8, 9]
    got_tokens, labels = w.random_word(tokens, None, 0)
    assert got_tokens is tokens and tokens == [7, 8, 9] and labels == [-1, -1, -1]
    feat, loc = np.arange(20, dtype=np.float32).reshape(5, 4), np.ones((5, 5), np.float32)
    ov = np.arange(9, dtype=np.float64).reshape(3, 3) / 10
    f, l, lab, slot = w.random_region(feat, loc, 3, 1, ov)
    assert f is feat and l is loc and lab == [-1, -1, -1]
    assert slot.dtype == np.float32 and slot.shape == (5, 5)
    assert np.array_equal(slot[:3, :3], ov.astype(np.float32)) and not slot[3:].any() and not slot[:, 3:].any()
    assert np.array_equal(feat, np.arange(20, dtype=np.float32).reshape(5, 4))
    f, l, lab, slot = w.random_region(feat, loc, 5, 0, np.ones((5, 5)))                # already [R, R]
    assert lab == [-1] * 5 and np.array_equal(slot, np.ones((5, 5), np.float32))
    assert ip.RAW_UNMASKED_FIELDS == mr.RAW_UNMASKED_FIELDS and ip.RAW_UNMASKED_FIELDS.index("overlaps") == ip.RAW_FIELDS.index("masked_label")
    assert [n for n in ip.RAW_UNMASKED_FIELDS if n != "overlaps"] == [n for n in ip.RAW_FIELDS if n != "masked_label"]


def test_reference_class_still_has_the_two_methods_with_those_parameters():
    from oracle import ref_loader
    path = os.path.join(ref_loader.REFERENCE_ROOT, "vilbert", "datasets", "concept_cap_dataset.py")
    if not os.path.isfile(path):
        pytest.skip("no reference checkout")
    tree = ast.parse(open(path).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BertPreprocessBatch"]
    assert len(cls) == 1
    params = {f.name: [a.arg for a in f.args.args] for f in cls[0].body if isinstance(f, ast.FunctionDef)}
    assert params["random_word"] == ["self", "tokens", "tokenizer", "is_next"]
    assert params["random_region"] == ["self", "image_feat", "image_loc", "num_boxes", "is_next", "overlaps"]
