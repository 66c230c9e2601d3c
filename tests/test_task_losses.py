"""Host side of the native fine-tuning loss and answer score (csrc/task_loss.hip, vilbert/task_losses.py): the header
include/vilbert_hip_tasks.h, its ctypes mirror and the built library agree, the three pinned headers are untouched, argument
errors come back without a GPU, CPU tensors fall through to torch bit for bit, and `vilbert.task_utils` is the reference's
module with its two criteria and its score function rebound. No compute is launched here; the GPU side is
tests/test_task_losses_gpu.py."""
import ctypes
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn as nn

from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vilbert-multi-task_amd")
TASK_HEADER = os.path.join(ROOT, "include", "vilbert_hip_tasks.h")
ENTRY_POINTS = ["vbt_argmax_pick", "vbt_bce_bwd", "vbt_bce_fwd", "vbt_bce_workspace"]
needs_reference = pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")

_C_TYPES = {"void*": ctypes.c_void_p, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
            "int": ctypes.c_int}
BADARG, RANGE = -1, -3


def _prototypes():
    """name -> (return ctype, [argument ctypes]) parsed from the header text; every pointer is a plain address."""
    text = re.sub(r"/\*.*?\*/", "", open(TASK_HEADER).read(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"\b(int64_t|int)\s+(vbt_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
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


def test_task_header_declares_exactly_the_four_entry_points_and_leaves_the_pinned_headers_alone():
    assert sorted(_prototypes()) == ENTRY_POINTS
    for name in ("vilbert_hip.h", "vilbert_hip_ext.h", "vilbert_hip_optim.h"):
        assert "vbt_" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "#define VB_ABI_VERSION 18" in open(os.path.join(ROOT, "include", "vilbert_hip.h")).read()


def test_ctypes_mirror_and_library_agree_with_the_task_header(native):
    protos = _prototypes()
    assert sorted(native.TASK_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.TASK_SIGNATURES[name][0] is res, name
        assert native.TASK_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbt_[a-z0-9_]+)", nm))) == ENTRY_POINTS
    lib = native.lib()
    assert lib.vb_abi_version() == 18
    for name in ENTRY_POINTS:                                  # bound with the mirrored types by lib()
        assert getattr(lib, name).argtypes == native.TASK_SIGNATURES[name][1]


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    a = ctypes.c_void_p(64)          # fake non-null addresses: the argument checks come before any launch
    # vbt_bce_fwd(stream, rows, n, logits, ld, target, ldt, workspace, loss)
    good = [None, 4, 3, a, 3, a, 3, a, a]
    for pos in (3, 5, 7, 8):                                   # each pointer null in turn
        args = list(good)
        args[pos] = None
        assert lib.vbt_bce_fwd(*args) == BADARG, pos
    assert lib.vbt_bce_fwd(None, 4, 0, a, 3, a, 3, a, a) == BADARG          # n <= 0
    assert lib.vbt_bce_fwd(None, 4, -2, a, 3, a, 3, a, a) == BADARG
    assert lib.vbt_bce_fwd(None, 4, 3, a, 2, a, 3, a, a) == BADARG          # ld < n
    assert lib.vbt_bce_fwd(None, 4, 3, a, 3, a, 2, a, a) == BADARG          # ldt < n
    assert lib.vbt_bce_fwd(None, -1, 3, a, 3, a, 3, a, a) == BADARG         # negative rows
    assert lib.vbt_bce_fwd(None, 1 << 40, 3, a, 1 << 40, a, 3, a, a) == RANGE   # rows * ld beyond int64
    assert lib.vbt_bce_fwd(None, 0, 3, a, 3, a, 3, a, a) == 0               # nothing to do: no launch
    # vbt_bce_bwd(stream, rows, n, logits, ld, target, ldt, grad_loss, dlogits, ldd)
    good = [None, 4, 3, a, 3, a, 3, a, a, 3]
    for pos in (3, 5, 7, 8):
        args = list(good)
        args[pos] = None
        assert lib.vbt_bce_bwd(*args) == BADARG, pos
    assert lib.vbt_bce_bwd(None, 4, 0, a, 3, a, 3, a, a, 3) == BADARG
    for pos in (4, 6, 9):                                      # each row stride < n in turn
        args = list(good)
        args[pos] = 2
        assert lib.vbt_bce_bwd(*args) == BADARG, pos
    assert lib.vbt_bce_bwd(None, -7, 3, a, 3, a, 3, a, a, 3) == BADARG
    assert lib.vbt_bce_bwd(None, 1 << 40, 3, a, 3, a, 3, a, a, 1 << 40) == RANGE
    assert lib.vbt_bce_bwd(None, 0, 3, a, 3, a, 3, a, a, 3) == 0
    # vbt_argmax_pick(stream, rows, n, logits, ld, labels, ldl, idx, picked, dense, ldo)
    good = [None, 4, 3, a, 3, a, 3, a, a, a, 3]
    for pos in (3, 5, 7, 8):                                   # dense (9) is optional
        args = list(good)
        args[pos] = None
        assert lib.vbt_argmax_pick(*args) == BADARG, pos
    assert lib.vbt_argmax_pick(None, 4, 0, a, 3, a, 3, a, a, None, 0) == BADARG
    for pos in (4, 6, 10):
        args = list(good)
        args[pos] = 2
        assert lib.vbt_argmax_pick(*args) == BADARG, pos
    assert lib.vbt_argmax_pick(None, -1, 3, a, 3, a, 3, a, a, None, 0) == BADARG
    assert lib.vbt_argmax_pick(None, 1 << 31, 3, a, 3, a, 3, a, a, None, 0) == RANGE
    assert lib.vbt_argmax_pick(None, 0, 3, a, 3, a, 3, a, a, None, 0) == 0
    assert lib.vbt_argmax_pick(None, 0, 3, a, 3, a, 3, a, a, a, 3) == 0


def test_workspace_is_one_float_per_block_of_the_forward(native):
    ws = native.lib().vbt_bce_workspace
    assert ws(0, 3) == 0 and ws(-1, 3) == 0 and ws(4, 0) == 0
    assert ws(256, 2) == 1 and ws(1025, 7) == 8                # flat mapping: 1024 elements per block
    assert ws(4, 255) == 1 and ws(5, 255) == 2
    assert ws(4, 256) == 4 and ws(300, 3129) == 300            # a block per row from n = 256 on
    assert ws(1 << 20, 3129) == 1024 and ws(1 << 30, 2) == 1024          # capped


def _upstream_score(logits, labels):
    """compute_score_with_logits as upstream writes it, without the `.cuda()`."""
    logits = torch.max(logits, 1)[1].data
    one_hots = torch.zeros(*labels.size())
    one_hots.scatter_(1, logits.view(-1, 1), 1)
    return one_hots * labels


def test_cpu_tensors_fall_back_to_torch_bit_for_bit():
    from vilbert import task_losses as TL
    g = torch.Generator().manual_seed(11)
    for shape in ((5, 3), (6, 3129), (4, 7, 1)):
        x = (torch.randn(*shape, generator=g) * 3).requires_grad_(True)
        t = torch.rand(*shape, generator=g)
        x2 = x.detach().clone().requires_grad_(True)
        got = TL.BCEWithLogitsLoss(reduction="mean")(x, t)
        want = nn.BCEWithLogitsLoss(reduction="mean")(x2, t)
        assert torch.equal(got, want) and type(got.grad_fn).__name__ == type(want.grad_fn).__name__
        (got * 1.7).backward()
        (want * 1.7).backward()
        assert torch.equal(x.grad, x2.grad)
    x = torch.randn(6, 4, generator=g, requires_grad=True)
    y = torch.tensor([0, 3, 1, -100, 2, 2])
    x2 = x.detach().clone().requires_grad_(True)
    got, want = TL.CrossEntropyLoss()(x, y), nn.CrossEntropyLoss()(x2, y)
    got.backward()
    want.backward()
    assert torch.equal(got, want) and torch.equal(x.grad, x2.grad)
    for shape in ((5, 3), (9, 2), (6, 3129)):
        logits, labels = torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)
        got = TL.compute_score_with_logits(logits, labels)
        assert got.dtype == torch.float32 and torch.equal(got, _upstream_score(logits, labels))
        idx, picked = TL.row_argmax_pick(logits, labels)
        assert idx.dtype == torch.int64 and torch.equal(idx, logits.argmax(1))
        assert torch.equal(picked, labels[torch.arange(shape[0]), idx])
    idx, picked = TL.row_argmax_pick(torch.randn(4, 7, 1, generator=g), torch.rand(4, 7, 1, generator=g))
    assert idx.shape == (4,) and picked.shape == (4,)


def test_modules_are_the_torch_modules():
    from vilbert import task_losses as TL
    bce, ce = TL.BCEWithLogitsLoss(reduction="mean"), TL.CrossEntropyLoss()
    assert isinstance(bce, nn.BCEWithLogitsLoss) and isinstance(ce, nn.CrossEntropyLoss)
    assert bce.reduction == "mean" and bce.pos_weight is None and ce.ignore_index == -100
    x, t = torch.zeros(2, 3), torch.zeros(2, 3)
    # every condition that keeps a call off the native path holds on the CPU
    assert not bce._native(x, t) and not ce._native(x, torch.zeros(2, dtype=torch.int64))
    assert not TL.BCEWithLogitsLoss(reduction="sum")._native(x, t)


def _run(code, cwd=None, **env):
    e = dict(os.environ)
    e.pop("PYTHONPATH", None)
    e.pop("VILBERT_REFERENCE_ROOT", None)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=e, cwd=cwd)


def test_without_a_reference_checkout_task_utils_stays_unimportable(tmp_path):
    code = ("import sys; sys.path.insert(0, %r); import vilbert\n"
            "assert vilbert.REFERENCE_PACKAGE_DIR is None\n"
            "try:\n    import vilbert.task_utils\nexcept ModuleNotFoundError as e:\n    print('MISSING', e.name)\n"
            "import vilbert.task_losses as TL; print('OK', TL.BCEWithLogitsLoss.__mro__[1].__name__)\n" % PKG)
    p = _run(code, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    assert "MISSING vilbert.task_utils" in p.stdout and "OK BCEWithLogitsLoss" in p.stdout


@needs_reference
def test_with_a_reference_checkout_task_utils_is_the_references_with_three_names_rebound():
    code = ("import sys, os; sys.path.insert(0, %r); import vilbert\n"
            "from vilbert import _compat; _compat.install(); sys.path.append(os.environ['VILBERT_REFERENCE_ROOT'])\n"
            "import torch.nn as nn, inspect, vilbert.task_utils as TU, vilbert.task_losses as TL\n"
            "assert sorted(TU.LossMap) == ['BCEWithLogitLoss', 'CrossEntropyLoss']\n"
            "bce, ce = TU.LossMap['BCEWithLogitLoss'], TU.LossMap['CrossEntropyLoss']\n"
            "assert type(bce) is TL.BCEWithLogitsLoss and type(ce) is TL.CrossEntropyLoss\n"
            "assert isinstance(bce, nn.BCEWithLogitsLoss) and isinstance(ce, nn.CrossEntropyLoss)\n"
            "assert bce.reduction == 'mean' and bce.pos_weight is None and ce.ignore_index == -100 and ce.reduction == 'mean'\n"
            "assert TU.compute_score_with_logits is TL.compute_score_with_logits\n"
            "assert TU.ForwardModelsTrain.__globals__['compute_score_with_logits'] is TL.compute_score_with_logits\n"
            "assert TU.ForwardModelsTrain.__globals__['LossMap'] is TU.LossMap\n"
            "assert 'def ForwardModelsTrain' in inspect.getsource(TU) and TU.LoadLosses.__module__ == 'vilbert.task_utils'\n"
            "print(TU.__file__)\n" % PKG)
    p = _run(code, VILBERT_REFERENCE_ROOT=ref_loader.REFERENCE_ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == os.path.join(ref_loader.REFERENCE_ROOT, "vilbert", "task_utils.py")
