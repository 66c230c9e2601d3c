"""Host side of the native multi-tensor RAdam step (csrc/optimizer.hip: radam_kernel; vilbert.optim.RAdam / PlainRAdam): the
new header include/vilbert_hip_optim.h, its ctypes mirror and the built library agree, argument errors come back without a
GPU, the host-side schedule (N_sma, rectified flag, step size, RAdam's step-size cache) reproduces the reference's own
classes, and checkpoints move between the implementations. No compute is launched here.

The golden trajectory tests/golden/radam_trajectory.npz was recorded from the REAL reference classes (the installed torch
still runs their `add_(scalar, tensor)` call forms; tests/golden/make_radam_golden.py). tests/radam_restatement.py restates
them; run in fp32 on the CPU it has to land on the recorded trajectory."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import radam_restatement as rr
from optim_helpers import C_TYPES as _C_TYPES, native, prototypes  # noqa: F401 (native: a fixture)
from oracle import ref_loader

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vilbert-multi-task_amd")
OPT_HEADER = os.path.join(ROOT, "include", "vilbert_hip_optim.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "radam_trajectory.npz")
needs_reference = pytest.mark.skipif(not ref_loader.available(), reason="reference tree not present")

# Distance between the restatement run in fp32 and in float64 on the fixture's case (max |p32 - p64| over the final
# parameters of both variants, measured: 2.83e-7; parameters are O(1), 12 steps). The recorded fp32 trajectory of the
# reference has to be met by the fp32 restatement within 4 x that - it is in fact met to the bit on the torch build the
# fixture was written with; the bound only leaves room for another CPU build contracting or vectorising differently.
GOLDEN_FP32_DISTANCE = 2.83e-7
GOLDEN_BOUND = 4 * GOLDEN_FP32_DISTANCE


def _prototypes():
    return prototypes(OPT_HEADER, "vbo_")


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_optimizer_header_declares_the_radam_entry_point_and_leaves_the_pinned_headers_alone():
    assert sorted(_prototypes()) == ["vbo_radam_step"]
    for name in ("vilbert_hip.h", "vilbert_hip_ext.h"):
        assert "vbo_" not in open(os.path.join(ROOT, "include", name)).read(), name
    assert "#define VB_ABI_VERSION 18" in open(os.path.join(ROOT, "include", "vilbert_hip.h")).read()


def test_ctypes_mirror_and_library_agree_with_the_optimizer_header(native):
    protos = _prototypes()
    assert sorted(native.OPT_SIGNATURES) == sorted(protos)
    for name, (res, args) in protos.items():
        assert native.OPT_SIGNATURES[name][0] is res, name
        assert native.OPT_SIGNATURES[name][1] == args, name
    nm = subprocess.run(["nm", "-D", "--defined-only", native.LIB_PATH], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r" T (vbo_[a-z0-9_]+)", nm))) == sorted(protos)
    # the per-tensor scalar table: field for field
    text = re.sub(r"/\*.*?\*/", "", open(OPT_HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct vbo_radam_scalars \{(.*?)\} vbo_radam_scalars;", text, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        fields += [(n.strip(), _C_TYPES[ctype]) for n in names.split(",")]
    assert fields == [(n, t) for n, t in native.RAdamScalars._fields_]
    assert ctypes.sizeof(native.RAdamScalars) == 32
    from vilbert import optim
    assert optim._RADAM_DTYPE.itemsize == 32 and list(optim._RADAM_DTYPE.names) == [n for n, _t in fields]
    assert native.lib().vb_abi_version() == 18


def test_argument_errors_do_not_need_a_gpu(native):
    lib = native.lib()
    a = ctypes.c_void_p(64)          # fake non-null addresses: the argument checks come before any launch
    assert lib.vbo_radam_step(None, 1, None, a, a, a, 65536, None, 0) == -1          # null table
    assert lib.vbo_radam_step(None, 1, a, None, a, a, 65536, None, 0) == -1          # null scalars
    assert lib.vbo_radam_step(None, 1, a, a, None, a, 65536, None, 0) == -1
    assert lib.vbo_radam_step(None, 1, a, a, a, None, 65536, None, 0) == -1
    assert lib.vbo_radam_step(None, 0, a, a, a, a, 65536, None, 0) == -1
    assert lib.vbo_radam_step(None, -5, a, a, a, a, 65536, a, 1) == -1
    # every chunk_elems vb_adamw_step refuses, with the same code
    for bad in (0, -4, 6, 65534):
        assert lib.vb_adamw_step(None, 1, a, a, a, bad) == -2
        assert lib.vbo_radam_step(None, 1, a, a, a, a, bad, None, 0) == -2
        assert lib.vbo_radam_step(None, 1, a, a, a, a, bad, a, 1) == -2


def test_fp32_restatement_lands_on_the_trajectory_recorded_from_the_reference(golden):
    meta = json.loads(str(golden["meta"]))
    assert meta["steps"] == rr.GOLDEN_STEPS and meta["sizes"] == list(rr.GOLDEN_SIZES)
    assert meta["source"].startswith("the reference's own vilbert.optimization.RAdam / PlainRAdam")
    p0, grads = rr.golden_inputs()
    worst = 0.0
    for name, plain in (("radam", False), ("plain", True)):
        r32 = rr.run_case(p0, grads, rr.GOLDEN_GROUPS, plain, torch.float32, rr.golden_lr_factor)
        r64 = rr.run_case(p0, grads, rr.GOLDEN_GROUPS, plain, torch.float64, rr.golden_lr_factor)
        assert r32.t == list(golden[name + "_steps"]) == [12, 10, 12]
        for i in range(3):
            for key, got in (("p", r32.p[i]), ("m", r32.m[i]), ("v", r32.v[i])):
                err = float(np.abs(got.numpy().astype(np.float64) - golden["%s_%s%d" % (name, key, i)]).max())
                assert err <= GOLDEN_BOUND, (name, key, i, err)
            worst = max(worst, float((r32.p[i].double() - r64.p[i]).abs().max()))
    print("fp32 vs float64 restatement on the fixture's case: max |diff| %.3e (recorded %.3e)" % (worst, GOLDEN_FP32_DISTANCE))
    assert worst <= 1.5 * GOLDEN_FP32_DISTANCE          # the figure the bound is built on still describes this case
    # both branches occur and the switch falls at step 6
    r = rr.run_case(p0, grads, rr.GOLDEN_GROUPS, True, torch.float64, rr.golden_lr_factor)
    assert {t for _i, t, n, _s in r.applied if n >= 5} == set(range(6, 13))
    assert {t for _i, t, n, _s in r.applied if n < 5} == set(range(1, 6))


def _drive_host_schedule(cls):
    """The native class's own `_fill_hyper` over the fixture's 12 steps, on the CPU: no launch, only the scalar table."""
    from vilbert import optim
    p0, grads = rr.golden_inputs()
    params = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = cls([{"params": [params[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}
               for g in rr.GOLDEN_GROUPS])
    base = [g["lr"] for g in opt.param_groups]
    rows, buffers = [], []
    for k, row in enumerate(grads):
        for g, lr in zip(opt.param_groups, base):
            g["lr"] = lr * rr.golden_lr_factor(k + 1)
        entries = []
        for group in opt.param_groups:
            for p in group["params"]:
                i = [q is p for q in params].index(True)
                if row[i] is None:
                    continue
                st = opt.state[p]
                st["step"] = st.get("step", 0) + 1
                entries.append((p, st, group, i))
        plan = {"extra": np.zeros(len(entries), dtype=optim._RADAM_DTYPE)}
        opt._fill_hyper(plan, [e[:3] for e in entries])
        for (_p, st, group, i), x in zip(entries, plan["extra"]):
            rows.append((i, st["step"], dict(zip(x.dtype.names, x.tolist())), group))
        if hasattr(opt, "buffer"):
            buffers.append([[np.nan if v is None else float(v) for v in slot] for slot in opt.buffer])
    return rows, np.array(buffers)


@pytest.mark.parametrize("name", ["radam", "plain"])
def test_host_schedule_reproduces_the_reference(name, golden):
    """Every row of the per-tensor scalar table over the 12 steps against the restatement (pinned above to the reference's
    trajectory): step size as the fp32 the kernel gets, rectified flag, lr * wd; and, for RAdam, the ten cache slots after
    every step against the `buffer` recorded from the reference class itself, as doubles."""
    from vilbert.optim import PlainRAdam, RAdam
    rows, buffers = _drive_host_schedule(RAdam if name == "radam" else PlainRAdam)
    p0, grads = rr.golden_inputs()
    r = rr.run_case(p0, grads, rr.GOLDEN_GROUPS, name == "plain", torch.float64, rr.golden_lr_factor)
    assert [(i, t) for i, t, _x, _g in rows] == [(i, t) for i, t, _n, _s in r.applied] and len(rows) == 34
    f32 = lambda x: float(np.float32(x))
    lr_of = {}
    for (i, t, x, group), (_i, _t, n, s) in zip(rows, r.applied):
        assert x["step_size"] == f32(s), (i, t)
        assert bool(x["rectified"]) == (n >= 5) == (t >= 6), (i, t)
        assert x["beta1"] == f32(0.9) and x["beta2"] == f32(0.999) and x["eps"] == f32(1e-8)
        assert x["one_minus_beta1"] == f32(1 - 0.9) and x["one_minus_beta2"] == f32(1 - 0.999)
        assert x["one_minus_beta2"] != f32(1) - f32(0.999)            # (what rounding the betas first would give)
        lr_of[(i, t)] = s
    # weight decay: each group's own lr * wd at the time of the step - never cached
    decays = {(i, x["decay"] != 0.0) for i, _t, x, _g in rows}
    assert decays == {(0, True), (1, True), (2, False)}
    if name == "radam":
        want = golden["radam_buffer"]
        assert buffers.shape == want.shape == (12, 10, 3)
        assert np.array_equal(np.isnan(buffers), np.isnan(want))
        assert np.allclose(buffers, want, rtol=1e-15, atol=0.0, equal_nan=True)
        # the quirk: tensor 2's group has lr 1e-5, yet it moves with the step size the lr-1e-3 group cached
        assert all(lr_of[(2, t)] == lr_of[(0, t)] for t in range(1, 13))
        assert lr_of[(2, 1)] == pytest.approx(1e-3 / (1 - 0.9), rel=1e-12)
        # tensor 1 fell behind at step 4: at its 4th step (the 5th call) it meets the slot filled one call earlier, under the older lr
        assert lr_of[(1, 4)] == lr_of[(0, 4)] == pytest.approx(1e-3 * rr.golden_lr_factor(4) / (1 - 0.9 ** 4), rel=1e-12)
    else:
        assert all(lr_of[(2, t)] == pytest.approx(lr_of[(0, t)] / 100.0, rel=1e-12) for t in range(1, 13))
        assert lr_of[(1, 4)] == pytest.approx(1e-3 * rr.golden_lr_factor(5) / (1 - 0.9 ** 4), rel=1e-12)


def test_constructor_and_defaults_are_the_references():
    from vilbert.optim import PlainRAdam, RAdam
    w = torch.nn.Parameter(torch.zeros(4))
    for cls in (RAdam, PlainRAdam):
        names = list(inspect.signature(cls.__init__).parameters)
        assert names[:6] == ["self", "params", "lr", "betas", "eps", "weight_decay"]
        opt = cls([w])
        assert opt.defaults == dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0)
        assert (opt.max_grad_norm, opt.grad_scale, opt.skip_nonfinite) == (0.0, 1.0, False) and not opt._scaled()
        assert opt.skipped_steps() == 0 and opt.last_step_skipped() is False
        with pytest.raises(RuntimeError, match="no clipped"):
            opt.grad_norm
        for bad in (dict(max_grad_norm=-1.0), dict(max_grad_norm=float("nan")), dict(grad_scale=float("inf"))):
            with pytest.raises(ValueError):
                cls([w], **bad)
        assert cls([w], max_grad_norm=1.0, skip_nonfinite=True)._scaled()
    assert len(RAdam([w]).buffer) == 10 and not hasattr(PlainRAdam([w]), "buffer")


@needs_reference
def test_constructor_signature_matches_the_reference_classes():
    import importlib
    from vilbert.optim import PlainRAdam, RAdam
    ref_loader.load()
    ref = importlib.import_module("vilbert_reference.optimization")
    for ours, theirs in ((RAdam, ref.RAdam), (PlainRAdam, ref.PlainRAdam)):
        want = list(inspect.signature(theirs.__init__).parameters.values())
        got = list(inspect.signature(ours.__init__).parameters.values())[:len(want)]
        assert [(p.name, p.default) for p in got] == [(p.name, p.default) for p in want]


def test_radam_has_no_cpu_fallback():
    from vilbert.optim import PlainRAdam, RAdam
    for cls in (RAdam, PlainRAdam):
        w = torch.nn.Parameter(torch.ones(8))
        w.grad = torch.ones(8)
        with pytest.raises(RuntimeError, match="HIP devices only"):
            cls([w]).step()
        w.grad = None
        assert cls([w]).step() is None and len(cls([w]).state) == 0          # nothing to do: no state, no launch


def _native_from_restatement(cls, r, p0):
    params = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = cls([{"params": [params[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}
               for g in rr.GOLDEN_GROUPS])
    opt.load_state_dict(r.state_dict())
    return opt, params


def test_checkpoint_layout_round_trips():
    """A state dict in the reference's layout (the restatement writes it) loads into the native class, comes back out with
    the reference's keys and loads again."""
    from vilbert.optim import PlainRAdam, RAdam
    p0, grads = rr.golden_inputs()
    r = rr.run_case(p0, grads, rr.GOLDEN_GROUPS, False, torch.float32, rr.golden_lr_factor)
    for cls in (RAdam, PlainRAdam):
        opt, params = _native_from_restatement(cls, r, p0)
        sd = opt.state_dict()
        assert set(sd) == {"state", "param_groups"} and sorted(sd["state"]) == [0, 1, 2]
        for k, i in enumerate([0, 1, 2]):
            assert set(sd["state"][k]) == {"step", "exp_avg", "exp_avg_sq"}
            assert sd["state"][k]["step"] == r.t[i] and torch.equal(sd["state"][k]["exp_avg"], r.m[i])
            assert torch.equal(sd["state"][k]["exp_avg_sq"], r.v[i])
        assert [set(g) for g in sd["param_groups"]] == [{"lr", "betas", "eps", "weight_decay", "params"}] * 2
        again, _ = _native_from_restatement(cls, r, p0)
        again.load_state_dict(sd)
        assert again.state_dict()["state"][1]["step"] == 10
        assert opt.state[params[1]]["exp_avg"].dtype == torch.float32


@needs_reference
def test_checkpoints_move_between_the_native_and_the_reference_classes():
    import importlib
    from vilbert.optim import PlainRAdam, RAdam
    ref_loader.load()
    ref = importlib.import_module("vilbert_reference.optimization")
    p0, grads = rr.golden_inputs()
    r = rr.run_case(p0, grads, rr.GOLDEN_GROUPS, False, torch.float32, rr.golden_lr_factor)
    for ours, theirs in ((RAdam, ref.RAdam), (PlainRAdam, ref.PlainRAdam)):
        opt, _params = _native_from_restatement(ours, r, p0)
        theirs_params = [torch.nn.Parameter(t.clone()) for t in p0]
        their_opt = theirs([{"params": [theirs_params[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}
                            for g in rr.GOLDEN_GROUPS])
        their_opt.load_state_dict(opt.state_dict())                      # native -> reference
        for p, g in zip(theirs_params, grads[0]):
            p.grad = g.clone()
        their_opt.step()                                                  # and the reference steps on it
        assert [their_opt.state[p]["step"] for p in theirs_params] == [13, 11, 13]
        back, _ = _native_from_restatement(ours, r, p0)
        back.load_state_dict(their_opt.state_dict())                      # reference -> native
        assert [back.state_dict()["state"][k]["step"] for k in range(3)] == [13, 11, 13]
        assert torch.equal(back.state_dict()["state"][0]["exp_avg"], their_opt.state[theirs_params[0]]["exp_avg"])


def _run(code, cwd=None, **env):
    e = dict(os.environ)
    e.pop("PYTHONPATH", None)
    e.pop("VILBERT_REFERENCE_ROOT", None)
    e.update(env)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=e, cwd=cwd)


def test_vilbert_optimization_offers_the_native_classes_without_a_reference_checkout(tmp_path):
    """`from vilbert.optimization import RAdam` (train_tasks.py:32) is the native class; without a reference checkout every
    other name of that module says what is missing."""
    code = ("import sys; sys.path.insert(0, %r); import vilbert, vilbert.optimization as o, vilbert.optim as n\n"
            "assert vilbert.REFERENCE_PACKAGE_DIR is None and len(vilbert.__path__) == 1\n"
            "assert o.RAdam is n.RAdam and o.PlainRAdam is n.PlainRAdam and o.__file__.startswith(%r)\n"
            "from vilbert.optimization import RAdam, PlainRAdam\n"
            "try:\n    o.required\nexcept AttributeError as e:\n    print('MSG', e)\n" % (PKG, PKG))
    p = _run(code, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-2000:]
    assert "VILBERT_REFERENCE_ROOT" in p.stdout


@needs_reference
def test_with_a_reference_checkout_the_module_is_the_references_with_the_two_classes_rebound():
    """The module stays the reference's own file - every other name of it as upstream - and only RAdam / PlainRAdam are the
    native classes."""
    code = ("import sys; sys.path.insert(0, %r); import vilbert, vilbert.optimization as o, vilbert.optim as n\n"
            "from vilbert.optimization import RAdam, PlainRAdam\n"
            "assert RAdam is n.RAdam and PlainRAdam is n.PlainRAdam and o.RAdam is n.RAdam\n"
            "import torch, torch.optim.optimizer as t, inspect\n"
            "assert o.required is t.required and o.clip_grad_norm_ is torch.nn.utils.clip_grad_norm_ and o.math.pi > 3\n"
            "assert 'class PlainRAdam' in inspect.getsource(o)\n"
            "print(o.__file__)\n" % PKG)
    p = _run(code, VILBERT_REFERENCE_ROOT=ref_loader.REFERENCE_ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert p.stdout.strip().splitlines()[-1] == os.path.join(ref_loader.REFERENCE_ROOT, "vilbert", "optimization.py")


def test_classes_carry_the_upstream_module_path_and_pickle_by_it():
    import pickle
    from vilbert.optim import PlainRAdam, RAdam
    for cls in (RAdam, PlainRAdam):
        assert cls.__module__ == "vilbert.optimization"
        blob = pickle.dumps(cls)
        assert b"vilbert.optimization" in blob and pickle.loads(blob) is cls
    w = torch.nn.Parameter(torch.zeros(3))
    back = pickle.loads(pickle.dumps(RAdam([w], lr=2e-3)))          # a whole optimizer object, as torch.save(optimizer) writes it
    assert type(back) is RAdam and back.param_groups[0]["lr"] == 2e-3 and len(back.buffer) == 10
