"""Host side of the single-stream baseline model (vilbert/basebert.py, csrc/joint_embed.hip): the module resolves to this
package without a reference checkout, its state_dict is the reference's (names and shapes pinned from the real reference by
tests/golden/make_basebert_golden.py), checkpoints load by the reference's key rules, the header
include/vilbert_hip_baseline.h, its ctypes mirror and the built library agree, and every documented argument error of the
`vbb_` entry points comes back without a GPU. No compute is launched here; the GPU side is tests/test_joint_embed_gpu.py and
tests/test_basebert_gpu.py."""
import ctypes
import json
import os
import re
import subprocess
import sys
import types

import pytest
import torch

import basebert_synth as BS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vilbert-multi-task_amd")
HEADER = os.path.join(ROOT, "include", "vilbert_hip_baseline.h")
ENTRY_POINTS = ["vbb_joint_embed_bwd", "vbb_joint_embed_bwd_workspace", "vbb_joint_embed_fwd", "vbb_tanh_bwd", "vbb_tanh_fwd",
                "vbb_text_embed_bwd"]
_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "int": ctypes.c_int}
BADARG, ALIGN, RANGE = -1, -2, -3


def _prototypes():
    """name -> (return ctype, [argument ctypes]) parsed from the header text; every pointer is a plain address."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbb_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
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


@pytest.fixture(scope="module")
def pinned_names():
    return [(k, tuple(s)) for k, s in json.load(open(BS.NAMES_JSON))]


def _tiny_model():
    from vilbert.basebert import BaseBertForVLTasks
    return BaseBertForVLTasks(BS.config("basebert_tiny"), num_labels=13)


def test_module_resolves_to_this_package_without_a_reference_checkout(tmp_path):
    code = ("import sys; sys.path.insert(0, %r); import vilbert\n"
            "assert vilbert.REFERENCE_PACKAGE_DIR is None\n"
            "import vilbert.basebert as B; print(B.__file__)\n"
            "from vilbert.basebert import (BertEmbeddings, BertImageEmbeddings, BertEncoder, BertPooler, BertPreTrainingHeads,\n"
            "    BertModel, BaseBertForVLTasks, BertForMultiModalPreTraining, BertLayerNorm, BertPreTrainedModel, SimpleClassifier)\n"
            % PKG)
    env = dict(os.environ)
    env.pop("PYTHONPATH", None)
    env.pop("VILBERT_REFERENCE_ROOT", None)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == os.path.join(PKG, "vilbert", "basebert.py")


def test_state_dict_has_the_references_names_and_shapes_and_the_decoder_is_tied(pinned_names):
    model = _tiny_model()
    sd = model.state_dict()
    assert len(pinned_names) == 72
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == pinned_names
    word = model.bert.embeddings.word_embeddings.weight
    assert model.cls.predictions.decoder.weight is word
    assert sd["cls.predictions.decoder.weight"].data_ptr() == sd["bert.embeddings.word_embeddings.weight"].data_ptr()
    for lin in (model.vil_prediction.main[0], model.vil_prediction.main[3]):
        assert lin.weight_g.dim() == 0 and lin.weight_v.shape == (lin.out_features, lin.in_features)


def test_the_pretraining_wrapper_constructs_with_the_references_names(pinned_names):
    from vilbert.basebert import BertForMultiModalPreTraining
    model = BertForMultiModalPreTraining(BS.config("basebert_tiny"))
    want = [k for k, _ in pinned_names if k.startswith(("bert.", "cls."))]
    assert list(model.state_dict()) == want
    with pytest.raises(NotImplementedError, match="864-866.*890"):
        model(None, None, None, None)


def test_any_config_object_with_the_attributes_is_accepted_and_checked_at_construction(pinned_names):
    import transformers
    from vilbert.basebert import BaseBertForVLTasks
    from vilbert.vilbert import BertConfig
    cfg = BS.CASES["basebert_tiny"]["cfg"]()
    for c in (transformers.BertConfig(**cfg), BertConfig.from_dict(cfg)):
        assert [(k, tuple(v.shape)) for k, v in BaseBertForVLTasks(c, 13).state_dict().items()] == pinned_names
    with pytest.raises(NotImplementedError, match="head size"):
        BaseBertForVLTasks(types.SimpleNamespace(**dict(cfg, num_attention_heads=4)), 13)      # 64 / 4 = 16
    with pytest.raises(NotImplementedError, match="activation"):
        BaseBertForVLTasks(types.SimpleNamespace(**dict(cfg, hidden_act="tanh")), 13)


def test_from_pretrained_round_trips_with_gamma_beta_and_prefixed_keys(tmp_path, pinned_names):
    from vilbert.basebert import BaseBertForVLTasks, BertModel
    cfg = BS.config("basebert_tiny")
    sd = BS.make_state_dict(pinned_names)
    # a checkpoint in the old naming: LayerNorm gamma / beta
    old = {k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta"): v for k, v in sd.items()}
    assert any("gamma" in k for k in old) and not any("LayerNorm.weight" in k for k in old)
    torch.save(old, str(tmp_path / "pytorch_model.bin"))
    model = BaseBertForVLTasks.from_pretrained(str(tmp_path), config=cfg, num_labels=13, default_gpu=True)
    got = model.state_dict()
    assert list(got) == [k for k, _ in pinned_names]
    for k, v in sd.items():
        assert torch.equal(got[k], v), k
    assert model.cls.predictions.decoder.weight is model.bert.embeddings.word_embeddings.weight
    # state_dict= and the optional `bert.` prefix: the bare BertModel takes the prefixed keys
    bare = BertModel.from_pretrained(None, config=cfg, state_dict=dict(old))
    for k, v in bare.state_dict().items():
        assert torch.equal(v, sd["bert." + k]), k
    assert BaseBertForVLTasks.from_pretrained(str(tmp_path / "missing"), config=cfg, num_labels=13) is None
    with pytest.raises(NotImplementedError):
        BaseBertForVLTasks.from_pretrained(str(tmp_path), config=cfg, from_tf=True, num_labels=13)


def test_set_active_heads_rejects_unknown_names_and_keeps_output_order():
    from vilbert import basebert
    model = _tiny_model()
    assert list(basebert.BASEBERT_HEADS) == BS.HEADS
    model.set_active_heads(["linguisic_logit", "vil_prediction"])
    assert model.active_heads == ("vil_prediction", "linguisic_logit")
    model.set_active_heads("vil_logit")
    assert model.active_heads == ("vil_logit",)
    model.set_active_heads(None)
    assert model.active_heads is None
    for bad in ("vil_prediction_gqa", ["vil_logit", "nope"]):          # (a head of the two-stream wrapper only)
        with pytest.raises(ValueError, match="unknown head"):
            model.set_active_heads(bad)


def test_half_raises():
    from vilbert.basebert import BertModel
    with pytest.raises(NotImplementedError, match="fp32"):
        _tiny_model().half()
    with pytest.raises(NotImplementedError, match="fp32"):
        BertModel(BS.config("basebert_tiny")).half()


def test_header_declares_exactly_the_six_entry_points_and_leaves_the_pinned_headers_alone():
    assert sorted(_prototypes()) == ENTRY_POINTS
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name != "vilbert_hip_baseline.h":
            assert "vbb_" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "#define VB_ABI_VERSION 18" in open(os.path.join(ROOT, "include", "vilbert_hip.h")).read()


def test_ctypes_mirror_and_library_agree_with_the_header(native):
    protos = _prototypes()
    assert sorted(native.BASELINE_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.BASELINE_SIGNATURES[name][0] is res, name
        assert native.BASELINE_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbb_[a-z0-9_]+)", nm))) == ENTRY_POINTS
    lib = native.lib()
    assert lib.vb_abi_version() == 18
    for name in ENTRY_POINTS:
        assert getattr(lib, name).argtypes == native.BASELINE_SIGNATURES[name][1]


A = ctypes.c_void_p(64)            # fake non-null 16-byte-aligned address: the argument checks come before any launch
ODD = ctypes.c_void_p(68)          # 4-byte aligned only

# vbb_joint_embed_fwd(stream, batch, n_tok, n_reg, hidden, vocab, n_types, ids, seg, word, pos, type, gamma_t, beta_t, feat_proj,
#                     loc, w_loc, b_loc, type_row, gamma_v, beta_v, eps, mask_t, f32, mask_v, f32, out, mean, rstd, presum, mask)
FWD = [None, 2, 3, 2, 8, 11, 2] + [A] * 14 + [1e-12, A, 0, A, 1, A, A, A, A, A]
FWD_REQUIRED = list(range(7, 21)) + [26, 30]
FWD_OPTIONAL = [22, 24, 27, 28, 29]
# vbb_joint_embed_bwd(stream, batch, n_tok, n_reg, hidden, dy, presum, mean, rstd, gamma_t, gamma_v, dx_text, dx_img, dgamma_t,
#                     dbeta_t, dgamma_v, dbeta_v, workspace)
BWD = [None, 2, 3, 2, 8] + [A] * 13
# vbb_text_embed_bwd(stream, batch, n_tok, hidden, vocab, n_types, n_tasks, ids, seg, task_ids, dx, dword, dpos, dtype, dtask,
#                    skip_pos0, skip_type0)
TBW = [None, 2, 3, 8, 11, 2, 0, A, A, None, A, A, A, A, None, 1, 1]


def _with(base, **at):
    args = list(base)
    for k, v in at.items():
        args[int(k[1:])] = v
    return args


def test_joint_embed_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    f, b = lib.vbb_joint_embed_fwd, lib.vbb_joint_embed_bwd
    for pos in FWD_REQUIRED:
        assert f(*_with(FWD, **{"p%d" % pos: None})) == BADARG, pos
    for pos in (2, 3, 4, 5, 6):                                            # n_tok, n_reg, hidden, vocab, n_types <= 0
        for v in (0, -1):
            assert f(*_with(FWD, **{"p%d" % pos: v})) == BADARG, (pos, v)
    assert f(*_with(FWD, p1=-1)) == BADARG                                 # negative batch
    assert f(*_with(FWD, p4=6)) == ALIGN                                   # hidden not a multiple of 4
    assert f(*_with(FWD, p4=8196)) == RANGE                                # hidden > VB_MAX_LN_COLS
    assert f(*_with(FWD, p1=(1 << 31) - 1, p2=(1 << 31) - 1, p3=(1 << 31) - 1, p4=8192)) == RANGE      # beyond int64
    for pos in (9, 10, 11, 12, 13, 14, 17, 18, 19, 20, 26, 29):            # the pointers read / written 16 bytes at a time
        assert f(*_with(FWD, **{"p%d" % pos: ODD})) == ALIGN, pos
    assert f(*_with(FWD, p1=0)) == 0                                       # zero rows: nothing launched
    assert f(*_with(FWD, p1=0, **{"p%d" % p: None for p in FWD_OPTIONAL})) == 0

    for pos in range(5, 18):
        assert b(*_with(BWD, **{"p%d" % pos: None})) == BADARG, pos
    for pos in (2, 3, 4):
        for v in (0, -1):
            assert b(*_with(BWD, **{"p%d" % pos: v})) == BADARG, (pos, v)
    assert b(*_with(BWD, p1=-1)) == BADARG
    assert b(*_with(BWD, p4=6)) == ALIGN
    assert b(*_with(BWD, p4=8196)) == RANGE
    assert b(*_with(BWD, p1=(1 << 31) - 1, p2=(1 << 31) - 1, p3=(1 << 31) - 1, p4=8192)) == RANGE
    for pos in (5, 6, 9, 10, 11, 12, 17):
        assert b(*_with(BWD, **{"p%d" % pos: ODD})) == ALIGN, pos
    assert b(*_with(BWD, p1=0)) == 0


def test_backward_workspace_is_one_partial_row_per_block_of_a_segment(native):
    ws = native.lib().vbb_joint_embed_bwd_workspace
    assert ws(0, 3, 2, 8) == 0 and ws(-1, 3, 2, 8) == 0 and ws(2, 0, 2, 8) == 0 and ws(2, 3, 2, 6) == 0
    assert ws(1, 1, 1, 4) == 2 * 2 * 4                                     # one block per segment
    assert ws(3, 7, 5, 64) == (2 + 1) * 2 * 64                             # 21 text rows: 2 blocks of 16; 15 image rows: 1
    assert ws(25, 7, 5, 768) == (11 + 8) * 2 * 768                         # 175 / 125 rows
    assert ws(2, 38, 101, 1024) == (5 + 13) * 2 * 1024
    assert ws(3, 7, 5, 1028) == (21 + 15) * 2 * 1028                       # wider than 1024: one partial per row


def test_text_embed_bwd_and_tanh_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    t = lib.vbb_text_embed_bwd
    for pos in (7, 8, 10, 11, 12, 13):
        assert t(*_with(TBW, **{"p%d" % pos: None})) == BADARG, pos
    for pos in (1, 2, 4, 5):
        assert t(*_with(TBW, **{"p%d" % pos: 0})) == BADARG, pos
    assert t(*_with(TBW, p9=A)) == BADARG                                  # task ids without a task table
    assert t(*_with(TBW, p3=0)) == BADARG and t(*_with(TBW, p3=6)) == ALIGN and t(*_with(TBW, p3=8196)) == RANGE
    assert t(*_with(TBW, p10=ODD)) == ALIGN
    # the same answers as the entry point it extends
    v = lib.vb_text_embed_bwd
    for at in ({"p7": None}, {"p1": 0}, {"p3": 6}, {"p3": 8196}, {"p10": ODD}, {"p9": A}):
        assert v(*_with(TBW, **at)[:15]) == t(*_with(TBW, **at)), at
    for fn, n_ptr in ((lib.vbb_tanh_fwd, 2), (lib.vbb_tanh_bwd, 3)):
        for pos in range(n_ptr):
            ptrs = [A] * n_ptr
            ptrs[pos] = None
            assert fn(None, 8, *ptrs) == BADARG, (fn, pos)
        assert fn(None, -1, *([A] * n_ptr)) == BADARG
        assert fn(None, 0, *([A] * n_ptr)) == 0
