"""Host side of the fused global-norm clipping / gradient scale / overflow-safe AdamW step (csrc/optimizer.hip): the
extension header declares the three entry points, the ctypes mirror and the built library agree with it, argument errors
come back without a GPU, and the optimizers accept and validate the new arguments. No compute is launched here.

The entry points carry the prefix `vbx_` and live in include/vilbert_hip_ext.h: tests/test_abi.py pins the export list of
include/vilbert_hip.h (header, ctypes mirror and `nm -D`) name by name at ABI 18."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from optim_helpers import native, prototypes  # noqa: F401 (native: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXT_HEADER = os.path.join(ROOT, "include", "vilbert_hip_ext.h")


def _prototypes():
    return prototypes(EXT_HEADER, "vbx_")


def test_extension_header_declares_the_three_entry_points():
    protos = _prototypes()
    assert sorted(protos) == ["vbx_adamw_step_scaled", "vbx_grad_norm", "vbx_grad_norm_workspace"]
    text = open(EXT_HEADER).read()
    assert int(re.search(r"#define VB_GRAD_STATE_FLOATS\s+(\d+)", text).group(1)) == 8
    main = open(os.path.join(ROOT, "include", "vilbert_hip.h")).read()
    assert "#define VB_ABI_VERSION 18" in main and "vbx_" not in main          # additive: the ABI-18 header is untouched


def test_ctypes_mirror_and_library_agree_with_the_extension_header(native):
    protos = _prototypes()
    assert sorted(native.EXT_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.EXT_SIGNATURES[name][0] is res, name
        assert native.EXT_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbx_[a-z0-9_]+)", nm))) == sorted(protos)
    text = open(EXT_HEADER).read()
    for key in ("FLOATS", "SUMSQ", "NORM", "COEF", "FINITE", "SKIPPED"):
        assert getattr(native, "GRAD_STATE_" + key) == int(re.search(r"#define VB_GRAD_STATE_%s\s+(\d+)" % key, text).group(1))
    assert native.lib().vb_abi_version() == 18


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    assert lib.vbx_grad_norm_workspace(0) == 0 and lib.vbx_grad_norm_workspace(-3) == 0
    assert lib.vbx_grad_norm_workspace(4321) == 4321                   # one fp32 partial per chunk
    assert lib.vbx_grad_norm(None, 1, None, None, None, 65536, 1.0, 1.0, 0, None, None) == -1
    assert lib.vbx_adamw_step_scaled(None, 1, None, None, None, 65536, None, 0) == -1
    # (fake non-null addresses: argument checks come before any launch)
    a = ctypes.c_void_p(64)
    assert lib.vbx_grad_norm(None, 0, a, a, a, 65536, 1.0, 1.0, 0, a, a) == -1
    assert lib.vbx_grad_norm(None, 1, a, a, a, 65536, -1.0, 1.0, 0, a, a) == -1
    assert lib.vbx_grad_norm(None, 1, a, a, a, 65536, float("nan"), 1.0, 0, a, a) == -1
    assert lib.vbx_grad_norm(None, 1, a, a, a, 65536, 1.0, float("inf"), 0, a, a) == -1
    assert lib.vbx_grad_norm(None, 1, a, a, a, 65534, 1.0, 1.0, 0, a, a) == -2
    assert lib.vbx_adamw_step_scaled(None, 1, a, a, a, 65536, None, 1) == -1
    assert lib.vbx_adamw_step_scaled(None, 1, a, a, a, 6, a, 1) == -2


def test_adamw_and_fusedadam_accept_and_validate_the_new_arguments():
    from apex.optimizers import FP16_Optimizer, FusedAdam
    from vilbert.optim import AdamW
    w = torch.nn.Parameter(torch.zeros(4))
    opt = AdamW([w])
    assert (opt.max_grad_norm, opt.grad_scale, opt.skip_nonfinite) == (0.0, 1.0, False) and not opt._scaled()
    opt = AdamW([w], max_grad_norm=1.0, grad_scale=0.125, skip_nonfinite=True)
    assert (opt.max_grad_norm, opt.grad_scale, opt.skip_nonfinite) == (1.0, 0.125, True) and opt._scaled()
    assert AdamW([w], grad_scale=0.5)._scaled() and AdamW([w], skip_nonfinite=True)._scaled()
    for bad in (dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan")), dict(grad_scale=float("inf")),
                dict(grad_scale=float("nan"))):
        with pytest.raises(ValueError):
            AdamW([w], **bad)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            FusedAdam([w], max_grad_norm=bad)
    assert opt.skipped_steps() == 0 and opt.last_step_skipped() is False          # nothing ran: no device read
    with pytest.raises(RuntimeError, match="no clipped"):
        opt.grad_norm
    # the defaults keep the checkpoint layout: nothing new in the state dict
    assert set(AdamW([w], max_grad_norm=1.0).state_dict()["param_groups"][0]) == set(AdamW([w]).state_dict()["param_groups"][0])

    fused = FusedAdam([w], lr=1e-3, bias_correction=False, max_grad_norm=1.0)
    assert fused.max_grad_norm == 1.0 and fused.skip_nonfinite and fused.grad_scale == 1.0
    assert FusedAdam([w]).skip_nonfinite and FusedAdam([w]).max_grad_norm == 0.0
    wrapped = FP16_Optimizer(fused, dynamic_loss_scale=True)
    assert wrapped.overflow is False and isinstance(type(wrapped).overflow, property)
    # clip_() stays public and works on plain (CPU) gradients: it no longer reaches into a gradient arena
    w.grad = torch.full((4,), 2.0)
    norm = fused.clip_()
    assert float(norm) == pytest.approx(4.0) and float(w.grad.norm()) == pytest.approx(1.0, rel=1e-5)
    assert FusedAdam([w]).clip_() is None
