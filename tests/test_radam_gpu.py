"""The native multi-tensor RAdam step (csrc/optimizer.hip: radam_kernel, vbo_radam_step; vilbert.optim.RAdam / PlainRAdam) on
the GPU: the 12-step trajectory against the float64 restatement (tests/radam_restatement.py) and against the trajectory
recorded from the reference's own classes (tests/golden/radam_trajectory.npz), RAdam's step-size cache, clipping and the
overflow skip through the device-resident state of vbx_grad_norm, the weights epoch / bf16 shadows, and the drop-in import.

Shapes: 1, 3 and 4 elements (scalar tail only / exactly one 16-byte access), 1021 (vector body + tail, more lanes than
elements in the last round), CHUNK_ELEMS + 5 (a second block whose chunk holds 5 elements) and a 37-element view one element
into its storage (4-byte but not 16-byte aligned: the scalar path for the whole tensor).

Tolerance (test 1, also used for the golden file and the clipped trajectory): the distance between the SAME restatement run
in fp32 torch on the CPU and in float64, on exactly this case, is max |diff| = 1.363e-6 on the parameters (O(1) values, the
largest of the 66,607 is 4.24, so this is 2.9 ulp there, after 12 steps of three roundings each), 1.925e-8 on exp_avg and
1.729e-9 on exp_avg_sq - measured once and recorded below; the fused kernel rounds in a different order than torch's
separate operations (it may contract a * b + c), so 4 x those figures are allowed: 5.45e-6, 7.7e-8 and 6.9e-9. The test
recomputes the fp32 - float64 distance and prints it next to the recorded figure. Over the 12 steps the parameters move by up
to 1.5e-2, 2,800 x the bound."""
import numpy as np
import os
import pytest
import torch

import radam_restatement as rr
from optim_helpers import DEV, bits_equal as _bits_equal, device_grad, device_params

pytestmark = pytest.mark.gpu
CHUNK = 65536
SIZES = [1, 3, 4, 1021, CHUNK + 5]
ODD = 37
# lr 1e-2 and beta2 = 0.98 (N_max = 99: the switch still falls at step 6, but the rectified step size reaches 0.08 lr at once
# instead of 0.003 lr with beta2 = 0.999): every term of the update - momentum step, rectified step, decay - moves the
# parameters by 1e-4 or more per step, far above the bound, so a wrong scalar or a wrong branch cannot hide under it
GROUPS = ({"idx": [0, 2, 4], "lr": 1e-2, "weight_decay": 0.01}, {"idx": [1, 3, 5], "lr": 1e-4, "weight_decay": 0.0})
BETAS = (0.9, 0.98)
MISSING = {(4, 3), (9, 3)}                  # (1-based step, tensor): no gradient
STEPS = 12
# measured fp32-vs-float64 distance of the restatement on this case (parameters, exp_avg, exp_avg_sq) and the bounds
DIST_P, DIST_M, DIST_V = 1.363e-6, 1.925e-8, 1.729e-9
BOUND_P, BOUND_M, BOUND_V = 4 * DIST_P, 4 * DIST_M, 4 * DIST_V
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "radam_trajectory.npz")


def _inputs(seed=77, scale=0.1, steps=STEPS, missing=MISSING):
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=g) for n in SIZES + [ODD]]
    grads = []
    for step in range(1, steps + 1):
        row = [torch.randn(n, generator=g) * scale for n in SIZES + [ODD]]
        grads.append([None if (step, i) in missing else t for i, t in enumerate(row)])
    return p0, grads


@pytest.fixture(scope="module")
def case():
    """Inputs and the float64 / fp32 CPU trajectories of both variants, computed once for the module (read-only)."""
    p0, grads = _inputs()
    out = {"p0": p0, "grads": grads}
    for name, plain in (("radam", False), ("plain", True)):
        out[name] = rr.run_case(p0, grads, GROUPS, plain, torch.float64, rr.golden_lr_factor, betas=BETAS)
        out[name + "32"] = rr.run_case(p0, grads, GROUPS, plain, torch.float32, rr.golden_lr_factor, betas=BETAS)
    return out


def _device_params(p0, odd_last=True):
    return device_params(p0, len(p0) - 1 if odd_last else None)


def _device_grad(t, i, n_tensors, odd_last=True):
    return device_grad(t, odd_last and i == n_tensors - 1)


def _make(cls, ps, groups=GROUPS, betas=BETAS, **kw):
    return cls([{"params": [ps[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups], betas=betas, **kw)


def _run_native(cls, p0, grads, groups=GROUPS, lr_factor=rr.golden_lr_factor, odd_last=True, **kw):
    ps = _device_params(p0, odd_last)
    opt = _make(cls, ps, groups, **kw)
    base = [g["lr"] for g in opt.param_groups]
    for k, row in enumerate(grads):
        if lr_factor is not None:
            for g, lr in zip(opt.param_groups, base):
                g["lr"] = lr * lr_factor(k + 1)
        for i, (p, t) in enumerate(zip(ps, row)):
            p.grad = _device_grad(t, i, len(ps), odd_last)
        opt.step()
    torch.cuda.synchronize()
    return opt, ps


def _worst(got, want):
    return max(float((a.detach().cpu().double() - b.double()).abs().max()) for a, b in zip(got, want))


@pytest.mark.parametrize("name", ["radam", "plain"])
def test_trajectory_matches_the_float64_restatement(name, case):
    """12 steps over both branches (momentum step up to step 5, rectified from step 6), two groups with different lr and
    weight decay, a shrinking lr, one tensor that misses two gradients. Measured distance fp32 restatement - float64:
    1.363e-6 / 1.925e-8 / 1.729e-9 (p / exp_avg / exp_avg_sq); bound = 4 x: 5.45e-6 / 7.7e-8 / 6.9e-9."""
    from vilbert.optim import PlainRAdam, RAdam
    r64, r32 = case[name], case[name + "32"]
    d = (_worst(r32.p, r64.p), _worst(r32.m, r64.m), _worst(r32.v, r64.v))
    print("%s: fp32 restatement vs float64: p %.3e  exp_avg %.3e  exp_avg_sq %.3e (recorded %.3e / %.3e / %.3e)"
          % ((name,) + d + (DIST_P, DIST_M, DIST_V)))
    opt, ps = _run_native(PlainRAdam if name == "plain" else RAdam, case["p0"], case["grads"])
    assert ps[-1].data_ptr() % 16 == 4 and opt._plan["n_chunks"] == len(ps) + 1
    got = (_worst(ps, r64.p), _worst([opt.state[p]["exp_avg"] for p in ps], r64.m),
           _worst([opt.state[p]["exp_avg_sq"] for p in ps], r64.v))
    print("%s: native vs float64: p %.3e  exp_avg %.3e  exp_avg_sq %.3e (bounds %.3e / %.3e / %.3e)"
          % ((name,) + got + (BOUND_P, BOUND_M, BOUND_V)))
    assert [opt.state[p]["step"] for p in ps] == r64.t == [12, 12, 12, 10, 12, 12]
    assert got[0] <= BOUND_P and got[1] <= BOUND_M and got[2] <= BOUND_V, got
    # the trajectory is not a trivial one: the parameters moved by far more than the bound
    assert _worst(r64.p, [t.double() for t in case["p0"]]) > 1e3 * BOUND_P


@pytest.mark.parametrize("name", ["radam", "plain"])
def test_final_parameters_of_the_references_own_trajectory_are_met(name):
    """The fixture recorded from the reference's RAdam / PlainRAdam (fp32, CPU), within the bound of the test above."""
    from vilbert.optim import PlainRAdam, RAdam
    z = np.load(GOLDEN)
    p0, grads = rr.golden_inputs()
    opt, ps = _run_native(PlainRAdam if name == "plain" else RAdam, p0, grads, groups=rr.GOLDEN_GROUPS, odd_last=False,
                          betas=(0.9, 0.999))
    want = [torch.from_numpy(z["%s_p%d" % (name, i)]) for i in range(3)]
    err = _worst(ps, want)
    print("%s: native vs the reference's recorded final parameters: %.3e (bound %.3e)" % (name, err, BOUND_P))
    assert err <= BOUND_P
    assert [opt.state[p]["step"] for p in ps] == list(z[name + "_steps"])
    assert _worst([opt.state[p]["exp_avg"] for p in ps], [torch.from_numpy(z["%s_m%d" % (name, i)]) for i in range(3)]) <= BOUND_M
    assert _worst([opt.state[p]["exp_avg_sq"] for p in ps], [torch.from_numpy(z["%s_v%d" % (name, i)]) for i in range(3)]) <= BOUND_V


def test_radam_moves_every_group_by_the_first_groups_step_size_plainradam_does_not():
    """Two groups, lr 1e-3 and 1e-5, the same values and the same gradients in both: under RAdam the cached step size of the
    first group moves the second by the same amount, bit for bit; under PlainRAdam the second moves 100 x less."""
    from vilbert.optim import PlainRAdam, RAdam
    g0 = torch.Generator().manual_seed(5)
    start = torch.zeros(1021)              # from zero: the fp32 rounding of p is relative to the move itself, not to an O(1) value
    grads = [torch.randn(1021, generator=g0) * 0.1 for _ in range(7)]          # crosses the switch at step 6
    moved = {}
    for cls in (RAdam, PlainRAdam):
        a, b = torch.nn.Parameter(start.to(DEV)), torch.nn.Parameter(start.to(DEV))
        opt = cls([{"params": [a], "lr": 1e-3}, {"params": [b], "lr": 1e-5}])
        for g in grads:
            a.grad, b.grad = g.to(DEV), g.to(DEV)
            opt.step()
        torch.cuda.synchronize()
        moved[cls] = (a.detach().cpu().double(), b.detach().cpu().double(), a, b)
    da, db, a, b = moved[RAdam]
    assert _bits_equal(a, b) and float(da.abs().max()) > 1e-4
    da, db, a, b = moved[PlainRAdam]
    assert not _bits_equal(a, b)
    big = da.abs() > 1e-5
    assert big.sum() > 900
    # the two step sizes differ by exactly 100 in double; seven fp32 accumulations of each leave a few 1e-7 relative
    assert float(((da[big] / db[big]) / 100.0 - 1.0).abs().max()) < 1e-4
    # and RAdam's first group moved exactly as PlainRAdam's first group (same lr, same schedule)
    assert _bits_equal(moved[RAdam][2], moved[PlainRAdam][2])


@pytest.mark.parametrize("name", ["radam", "plain"])
def test_clipped_step_equals_the_plain_step_on_gradients_scaled_by_torchs_coefficient(name):
    from vilbert.optim import PlainRAdam, RAdam
    cls = PlainRAdam if name == "plain" else RAdam
    p0, grads = _inputs(seed=78, scale=0.5, steps=8, missing={(3, 3)})
    max_norm = 1.0
    ps, qs = _device_params(p0), _device_params(p0)
    clipped, plain = _make(cls, ps, max_grad_norm=max_norm), _make(cls, qs)
    for row in grads:
        keep = []
        for i, (p, q, t) in enumerate(zip(ps, qs, row)):
            p.grad, q.grad = _device_grad(t, i, len(ps)), _device_grad(t, i, len(ps))
            keep.append(None if t is None else p.grad.clone())
        used = [q for q in qs if q.grad is not None]
        norm = torch.nn.utils.clip_grad_norm_(used, max_norm)
        assert float(norm) > 50.0                                        # the clipping is active
        clipped.step()
        plain.step()
        assert abs(clipped.grad_norm.item() - float(norm)) <= 2e-5 * float(norm)
        for p, k in zip(ps, keep):
            assert k is None or _bits_equal(p.grad, k), "step() modified a gradient"
    torch.cuda.synchronize()
    err = (_worst(ps, [q.detach().cpu() for q in qs]),
           _worst([clipped.state[p]["exp_avg"] for p in ps], [plain.state[q]["exp_avg"].cpu() for q in qs]),
           _worst([clipped.state[p]["exp_avg_sq"] for p in ps], [plain.state[q]["exp_avg_sq"].cpu() for q in qs]))
    print("%s clipped vs clip_grad_norm_ + plain: p %.3e exp_avg %.3e exp_avg_sq %.3e" % ((name,) + err))
    assert err[0] <= BOUND_P and err[1] <= BOUND_M and err[2] <= BOUND_V, err
    assert clipped.skipped_steps() == 0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step(bad):
    from vilbert.optim import RAdam
    p0, grads = _inputs(seed=79, steps=3, missing=set())
    ps = _device_params(p0)
    opt = _make(RAdam, ps, skip_nonfinite=True)
    for i, (p, t) in enumerate(zip(ps, grads[0])):
        p.grad = _device_grad(t, i, len(ps))
    opt.step()
    assert opt.skipped_steps() == 0 and not opt.last_step_skipped()
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    for i, (p, t) in enumerate(zip(ps, grads[1])):
        p.grad = _device_grad(t, i, len(ps))
    ps[4].grad[CHUNK + 2].fill_(bad)                  # one element, in the second chunk of one gradient
    opt.step()
    torch.cuda.synchronize()
    for p, (p_, m_, v_) in zip(ps, before):
        assert _bits_equal(p, p_) and _bits_equal(opt.state[p]["exp_avg"], m_) and _bits_equal(opt.state[p]["exp_avg_sq"], v_)
    assert opt.skipped_steps() == 1 and opt.last_step_skipped()
    for i, (p, t) in enumerate(zip(ps, grads[2])):
        p.grad = _device_grad(t, i, len(ps))
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and not opt.last_step_skipped()
    assert all(torch.isfinite(p).all() for p in ps) and not _bits_equal(ps[4], before[4][0])


def test_step_advances_the_weights_epoch_and_a_bf16_forward_sees_the_new_weights():
    from vilbert import _native, ops16
    from vilbert.optim import RAdam
    g0 = torch.Generator().manual_seed(9)
    w = torch.nn.Parameter((torch.randn(128, 64, generator=g0) * 0.1).to(DEV))     # (the bf16 GEMM wants N % 128 == 0, K % 64 == 0)
    x = torch.randn(128, 64, generator=g0).to(DEV).to(torch.bfloat16)
    opt = RAdam([w], lr=0.05)                                   # first step: p -= lr / (1 - 0.9) * 0.1 g = 0.05 g
    y0 = ops16.linear_fwd(x, [w], [None])[0].float()
    w.grad = torch.randn(128, 64, generator=g0).to(DEV)
    e0, v0 = _native.WEIGHTS_EPOCH[0], w._version
    opt.step()
    assert _native.WEIGHTS_EPOCH[0] > e0 and w._version == v0    # (raw-pointer writes: only the epoch can tell)
    y1 = ops16.linear_fwd(x, [w], [None])[0].float()
    torch.cuda.synchronize()
    want = x.float() @ w.detach().to(torch.bfloat16).float().t()
    assert float((y1 - y0).abs().max()) > 0.1                    # the weights moved visibly ...
    assert float((y1 - want).abs().max()) <= 2 ** -7 * float(want.abs().max()) + 1e-3       # ... and the forward used them
    if opt._arena is not None:
        opt._arena.release()


def test_drop_in_import_and_reference_layout_checkpoint(case):
    """`from vilbert.optimization import RAdam` is the native class; a state dict in the reference's layout, written by the
    float64 restatement half-way, loads into it and the continued trajectory ends where the uninterrupted one does."""
    from vilbert import optim
    from vilbert.optimization import PlainRAdam, RAdam
    assert RAdam is optim.RAdam and PlainRAdam is optim.PlainRAdam
    p0, grads = case["p0"], case["grads"]
    half = rr.Restatement([t.double() for t in p0], GROUPS, betas=BETAS)
    base = [g["lr"] for g in half.groups]
    for k in range(6):
        for g, lr in zip(half.groups, base):
            g["lr"] = lr * rr.golden_lr_factor(k + 1)
        half.step([None if t is None else t.double() for t in grads[k]])
    ps = _device_params([t.float() for t in half.p])
    opt = _make(RAdam, ps)
    opt.load_state_dict(half.state_dict())
    assert all(opt.state[p]["exp_avg"].dtype == torch.float32 and opt.state[p]["exp_avg"].is_cuda for p in ps)
    opt.buffer = [list(s) for s in half.slots]                  # (the cache is not part of a checkpoint, upstream neither)
    for k in range(6, STEPS):
        for g, lr in zip(opt.param_groups, base):
            g["lr"] = lr * rr.golden_lr_factor(k + 1)
        for i, (p, t) in enumerate(zip(ps, grads[k])):
            p.grad = _device_grad(t, i, len(ps))
        opt.step()
    torch.cuda.synchronize()
    err = _worst(ps, case["radam"].p)
    print("resumed from a reference-layout checkpoint: native vs float64 %.3e (bound %.3e)" % (err, BOUND_P))
    assert err <= BOUND_P
    assert set(opt.state_dict()["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
