"""The native LAMB step (csrc/lamb.hip: lamb_stage1_kernel, lamb_stage2_kernel, vbl_lamb_step; vilbert.optim.LAMB,
apex.optimizers.FusedLAMB) on the GPU, against the float64 restatement (tests/lamb_restatement.py).

Tensors (the case of tests/lamb_restatement.py, 268,598 elements): 1 element; 5 elements as a view one element into its
storage (data_ptr % 16 == 4: the scalar path for the whole tensor); 65536 + 7 (two chunks, the second with one 16-byte access
and a scalar tail); 3 x 65536 (three full chunks between two neighbours: first_chunk); an all-zero parameter with a non-zero
gradient (||p|| = 0 -> r = 1); a tensor with zero gradients and zero moments in the group without decay (||u|| = 0, p does not
move); a tensor of the group without decay (r = 1 exactly unless use_nvlamb); a tensor that misses its gradient on steps 4
and 9. The gradients are drawn at a scale of 0.1 on odd steps (global norm about 52: clipped) and 1e-3 on even ones (about
0.5: not clipped).

Tolerances: the distance between the SAME restatement run in fp32 torch on the CPU and in float64 on exactly this case,
measured and recorded per configuration in tests/test_lamb.py (DIST; e.g. 1.015e-6 / 3.464e-10 / 4.203e-14 on parameters /
exp_avg / exp_avg_sq with the defaults); the fused kernels round in another order than torch's separate operations (they may
contract a * b + c), so 4 x those figures are allowed - the rule of tests/test_radam_gpu.py. Every test prints what it measured
next to its bound."""
import pytest
import torch

import lamb_restatement as lamb
from optim_helpers import DEV, bits_equal as _bits_equal, device_grad, device_params
from optim_helpers import leave_no_workspace_slices_behind  # noqa: F401 (an autouse fixture: the captured step and the model of this file bring streams of their own)
from test_lamb import DIST, options, worst

pytestmark = pytest.mark.gpu
CHUNK = lamb.CHUNK
N_CHUNKS = 1 + 1 + 2 + 3 + 1 + 1 + 1 + 1
WALK = [i for g in lamb.GROUPS for i in g["idx"]]           # the order step() walks the tensors in: groups, then parameters
IDS = lambda c: "%s-%s-%s" % ("adamw" if c[0] else "l2", "corrected" if c[1] else "plain", "averaged" if c[2] else "summed")


@pytest.fixture(scope="module")
def case():
    """Inputs of the trajectory case, computed once for the module (read-only)."""
    p0, grads = lamb.inputs()
    return {"p0": p0, "grads": grads}


def _device_params(p0):
    return device_params(p0, lamb.ODD)


def _device_grad(t, i):
    return device_grad(t, i == lamb.ODD)


def _make(cls, ps, groups=lamb.GROUPS, **kw):
    return cls([{"params": [ps[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]} for g in groups], **kw)


def _run_native(cls, p0, grads, groups=lamb.GROUPS, factor=lamb.lr_factor, **kw):
    ps = _device_params(p0)
    opt = _make(cls, ps, groups, **kw)
    base = [g["lr"] for g in opt.param_groups]
    for k, row in enumerate(grads):
        if factor is not None:
            for g, lr in zip(opt.param_groups, base):
                g["lr"] = lr * factor(k + 1)
        for i, (p, t) in enumerate(zip(ps, row)):
            p.grad = _device_grad(t, i)
        opt.step()
    torch.cuda.synchronize()
    return opt, ps


def _state(opt, ps):
    return [p.detach().clone() for p in ps] + [opt.state[p][k].clone() for k in ("exp_avg", "exp_avg_sq") for p in ps]


def _release(*opts):
    for opt in opts:
        if opt._arena is not None:
            opt._arena.release()


@pytest.mark.parametrize("config", lamb.CONFIGS, ids=IDS)
def test_trajectory_matches_the_float64_restatement(config, case):
    """12 steps, two groups with different lr and decay, a shrinking lr, clipping active on every other step, one tensor that
    misses two gradients; decoupled / L2 decay x bias correction x gradient averaging. Bounds: 4 x DIST[config] of
    tests/test_lamb.py."""
    from vilbert.optim import LAMB
    r64 = lamb.run_case(case["p0"], case["grads"], lamb.GROUPS, torch.float64, lamb.lr_factor, max_grad_norm=lamb.MAX_GRAD_NORM,
                        **options(config))
    bound = tuple(4 * d for d in DIST[config])
    opt, ps = _run_native(LAMB, case["p0"], case["grads"], max_grad_norm=lamb.MAX_GRAD_NORM, **options(config))
    assert ps[lamb.ODD].data_ptr() % 16 == 4 and opt._plan["n_chunks"] == N_CHUNKS
    got = (worst(ps, r64.p), worst([opt.state[p]["exp_avg"] for p in ps], r64.m),
           worst([opt.state[p]["exp_avg_sq"] for p in ps], r64.v))
    print("%s: fp32 restatement vs float64 (recorded): p %.3e  exp_avg %.3e  exp_avg_sq %.3e" % ((IDS(config),) + DIST[config]))
    print("%s: native vs float64: p %.3e  exp_avg %.3e  exp_avg_sq %.3e (bounds %.3e / %.3e / %.3e)" % ((IDS(config),) + got + bound))
    assert [opt.state[p]["step"] for p in ps] == r64.t == [12] * 7 + [10]
    assert got[0] <= bound[0] and got[1] <= bound[1] and got[2] <= bound[2], got
    # the trajectory is not a trivial one: the parameters moved by far more than the bound
    assert worst(r64.p, case["p0"]) > 1e3 * bound[0]
    assert _bits_equal(ps[lamb.ZERO_GRAD], case["p0"][lamb.ZERO_GRAD].to(DEV))             # ||u|| = 0: p never moved
    assert opt.skipped_steps() == 0
    _release(opt)


@pytest.mark.parametrize("use_nvlamb", [False, True], ids=["lamb", "nvlamb"])
def test_trust_ratios_after_one_step_match_the_float64_norms(use_nvlamb, case):
    """r = ||p|| / ||u|| of every tensor, from the same inputs in float64. Relative bound: 4 x the largest relative error of
    the fp32 restatement's ratios on these tensors, measured here (about 1e-7). Exactly 1.0: the all-zero parameter, the tensor
    with ||u|| = 0 (under use_nvlamb it has apply_trust set and takes the norm branch), and - without use_nvlamb - the
    tensors of the group without decay."""
    from vilbert.optim import LAMB
    one = case["grads"][:1]
    r64 = lamb.run_case(case["p0"], one, lamb.GROUPS, torch.float64, None, use_nvlamb=use_nvlamb)
    r32 = lamb.run_case(case["p0"], one, lamb.GROUPS, torch.float32, None, use_nvlamb=use_nvlamb)
    assert r64.order == WALK
    own = max(abs(r32.trust[i] / r64.trust[i] - 1.0) for i in WALK)
    bound = 4 * own
    opt, ps = _run_native(LAMB, case["p0"], one, factor=None, use_nvlamb=use_nvlamb)
    got = opt.trust_ratios
    assert got.is_cuda and got.shape == (len(WALK),) and got.dtype == torch.float32
    got = got.cpu().double().tolist()
    rel = max(abs(g / r64.trust[i] - 1.0) for g, i in zip(got, WALK))
    print("trust ratios (use_nvlamb=%s): native %s\n  float64 %s\n  fp32 restatement off by %.3e, native off by %.3e (bound %.3e)"
          % (use_nvlamb, got, [r64.trust[i] for i in WALK], own, rel, bound))
    assert 0.0 < own < 1e-6 and rel <= bound
    exact = [lamb.ZERO_PARAM, lamb.ZERO_GRAD] + ([] if use_nvlamb else [lamb.NO_DECAY])
    for i in exact:
        assert got[WALK.index(i)] == 1.0 == r64.trust[i], i
    assert all(got[WALK.index(i)] != 1.0 for i in set(WALK) - set(exact))
    for i in WALK:
        view = opt.trust_ratio(ps[i])
        assert view.dim() == 0 and view.data_ptr() == opt.trust_ratios[WALK.index(i)].data_ptr()
    with pytest.raises(KeyError):
        opt.trust_ratio(torch.nn.Parameter(torch.zeros(1, device=DEV)))
    _release(opt)


def test_same_inputs_give_the_same_bits_wherever_a_tensor_stands(case):
    """Two runs of four clipped steps: identical bits in p, m, v and the trust ratios. Then the three-chunk tensor and the
    lagging one move to the front of their group (every first_chunk changes): each tensor's bits stay what they were. The
    moved runs are unclipped ones: a tensor's bits depend on its own values and on the clip coefficient, and the coefficient
    comes from a sum over all chunks in table order - a global quantity that the order may move by an ulp, whatever the
    optimizer."""
    from vilbert.optim import LAMB
    grads = case["grads"][:4]
    a, pa = _run_native(LAMB, case["p0"], grads)
    b, pb = _run_native(LAMB, case["p0"], grads)
    assert all(_bits_equal(x, y) for x, y in zip(_state(a, pa), _state(b, pb)))
    assert _bits_equal(a.trust_ratios, b.trust_ratios) and _bits_equal(a.grad_norm, b.grad_norm)
    moved = ({"idx": [3, 7, 0, 1, 2, 4], "lr": 1e-2, "weight_decay": 0.01}, {"idx": [6, 5], "lr": 1e-3, "weight_decay": 0.0})
    c, pc = _run_native(LAMB, case["p0"], grads, max_grad_norm=0.0)
    d, pd = _run_native(LAMB, case["p0"], grads, groups=moved, max_grad_norm=0.0)
    assert list(d._plan["extra"]["first_chunk"]) != list(c._plan["extra"]["first_chunk"])
    assert all(_bits_equal(x, y) for x, y in zip(_state(c, pc), _state(d, pd)))
    for i in range(len(pc)):
        if i == lamb.LAGGING:                         # the fourth step had no gradient for it: it is not in the last plan
            with pytest.raises(KeyError):
                c.trust_ratio(pc[i])
            continue
        assert _bits_equal(c.trust_ratio(pc[i]), d.trust_ratio(pd[i])), i
    assert len(c.trust_ratios) == len(d.trust_ratios) == 7
    assert not _bits_equal(pa[3], pc[3])                                                 # (the clipping did act in the first pair)
    _release(a, b, c, d)


def test_clipped_step_equals_the_plain_step_on_gradients_scaled_by_torchs_coefficient():
    """The form of tests/test_radam_gpu.py's test of that name: eight steps at a gradient scale of 0.5 (global norm about
    260), the clipped optimizer against clip_grad_norm_ followed by the unclipped one, within the bounds of the trajectory
    test; step() leaves every .grad bit-unchanged."""
    from vilbert.optim import LAMB
    bound = tuple(4 * d for d in DIST[(True, True, True)])
    p0, grads = lamb.inputs(seed=78, steps=8, missing={(3, lamb.LAGGING)}, scales=(0.5,))
    max_norm = 1.0
    ps, qs = _device_params(p0), _device_params(p0)
    clipped, plain = _make(LAMB, ps, max_grad_norm=max_norm), _make(LAMB, qs, max_grad_norm=0.0)
    for row in grads:
        keep = []
        for i, (p, q, t) in enumerate(zip(ps, qs, row)):
            p.grad, q.grad = _device_grad(t, i), _device_grad(t, i)
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
    err = (worst(ps, qs), worst([clipped.state[p]["exp_avg"] for p in ps], [plain.state[q]["exp_avg"] for q in qs]),
           worst([clipped.state[p]["exp_avg_sq"] for p in ps], [plain.state[q]["exp_avg_sq"] for q in qs]))
    print("clipped vs clip_grad_norm_ + plain: p %.3e exp_avg %.3e exp_avg_sq %.3e (bounds %.3e / %.3e / %.3e)" % (err + bound))
    assert err[0] <= bound[0] and err[1] <= bound[1] and err[2] <= bound[2], err
    assert clipped.skipped_steps() == 0 and worst(ps, p0) > 1e3 * bound[0]
    _release(clipped, plain)


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step(bad):
    from vilbert.optim import LAMB
    p0, grads = lamb.inputs(seed=79, steps=3, missing=set())
    ps = _device_params(p0)
    opt = _make(LAMB, ps, skip_nonfinite=True)

    def step(row):
        for i, (p, t) in enumerate(zip(ps, row)):
            p.grad = _device_grad(t, i)
    step(grads[0])
    opt.step()
    assert opt.skipped_steps() == 0 and not opt.last_step_skipped()
    before, trust = _state(opt, ps), opt.trust_ratios.clone()
    step(grads[1])
    ps[2].grad[CHUNK + 2].fill_(bad)                  # one element, in the second chunk of one gradient
    opt.step()
    torch.cuda.synchronize()
    assert all(_bits_equal(x, y) for x, y in zip(_state(opt, ps), before)) and _bits_equal(opt.trust_ratios, trust)
    assert opt.skipped_steps() == 1 and opt.last_step_skipped()
    step(grads[2])
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and not opt.last_step_skipped()
    assert all(torch.isfinite(p).all() for p in ps) and not _bits_equal(ps[2], before[2])
    assert not _bits_equal(opt.trust_ratios, trust) and [opt.state[p]["step"] for p in ps] == [3] * 8
    _release(opt)


def test_captured_step_replays_the_eager_trajectory_bit_for_bit():
    """Five steps with every gradient in the optimizer's arena (fixed addresses): eagerly, and as two eager steps, a capture
    of opt.step() on one stream and three replays behind prepare_replay(), with the learning rate shrinking from step to
    step. The capture executes nothing on the device but advances the host-side step counts, which the test takes back (as
    GraphedTrainStep does)."""
    from vilbert import arena as A
    from vilbert.optim import LAMB
    p0, grads = lamb.inputs(seed=80, steps=5, missing=set())

    def load(opt, ps, row, k):
        for g, lr in zip(opt.param_groups, base):
            g["lr"] = lr * lamb.lr_factor(k + 1)
        for p, t in zip(ps, row):
            index = A.lookup(p)[1]
            opt._arena.views[index].copy_(t)
            p.grad = opt._arena.alias(index)

    ps = _device_params(p0)
    eager = _make(LAMB, ps)
    base = [g["lr"] for g in eager.param_groups]
    assert eager._arena is not None
    for k, row in enumerate(grads):
        load(eager, ps, row, k)
        eager.step()
    torch.cuda.synchronize()
    want, want_trust = _state(eager, ps), eager.trust_ratios.clone()
    _release(eager)

    qs = _device_params(p0)
    opt = _make(LAMB, qs)
    for k in range(2):
        load(opt, qs, grads[k], k)
        opt.step()
    torch.cuda.synchronize()
    load(opt, qs, grads[2], 2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for q in qs:
        opt.state[q]["step"] -= 1
    trust = opt.trust_ratios
    for k in range(2, 5):
        load(opt, qs, grads[k], k)
        torch.cuda.synchronize()                      # the previous replay is done with the pinned table
        opt.prepare_replay()
        graph.replay()
    torch.cuda.synchronize()
    assert [opt.state[q]["step"] for q in qs] == [5] * 8
    assert all(_bits_equal(x, y) for x, y in zip(_state(opt, qs), want))
    assert _bits_equal(trust, want_trust) and trust.data_ptr() == opt.trust_ratios.data_ptr()
    del graph
    _release(opt)


def test_step_advances_the_weights_epoch_and_a_bf16_forward_sees_the_new_weights():
    """The form of tests/test_radam_gpu.py's test of that name. First LAMB step: u = sign(g) + 0.01 p to within eps, so
    r = ||p|| / ||u|| is about 0.1 and every weight moves by about lr r = 0.05."""
    from vilbert import _native, ops16
    from vilbert.optim import LAMB
    g0 = torch.Generator().manual_seed(9)
    w = torch.nn.Parameter((torch.randn(128, 64, generator=g0) * 0.1).to(DEV))     # (the bf16 GEMM wants N % 128 == 0, K % 64 == 0)
    x = torch.randn(128, 64, generator=g0).to(DEV).to(torch.bfloat16)
    opt = LAMB([w], lr=0.5)
    y0 = ops16.linear_fwd(x, [w], [None])[0].float()
    w.grad = torch.randn(128, 64, generator=g0).to(DEV)
    e0, v0 = _native.WEIGHTS_EPOCH[0], w._version
    opt.step()
    assert _native.WEIGHTS_EPOCH[0] > e0 and w._version == v0    # (raw-pointer writes: only the epoch can tell)
    y1 = ops16.linear_fwd(x, [w], [None])[0].float()
    torch.cuda.synchronize()
    want = x.float() @ w.detach().to(torch.bfloat16).float().t()
    assert 0.05 < float(opt.trust_ratio(w)) < 0.2
    assert float((y1 - y0).abs().max()) > 0.1                    # the weights moved visibly ...
    assert float((y1 - want).abs().max()) <= 2 ** -7 * float(want.abs().max()) + 1e-3       # ... and the forward used them
    _release(opt)


def test_fused_lamb_inside_fp16_optimizer_trains_the_tiny_model_in_bf16_mode():
    """Three steps of the tiny pre-training model on a fixed batch, dropout off, bf16 mode: every loss finite, none above
    the one before it, and the loss after the three steps below the first."""
    import vilbert.vilbert as V
    from apex.optimizers import FP16_Optimizer, FusedLAMB
    from oracle import synth
    from vilbert import _native
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    names = ["input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
             "masked_lm_labels", "image_label", "image_target", "next_sentence_label"]
    cfg = synth.tiny_config()
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
    model.load_state_dict(synth.make_state_dict(cfg, "pretraining"))
    model = model.to(DEV).train()
    x = synth.make_inputs(cfg, 4, 9, 8, with_labels=True)
    args = [x[n].to(DEV) for n in names]
    orig, V._drop_p = V._drop_p, (lambda m: 0.0)
    prev = _native.set_gemm_mode("bf16")
    fused = FusedLAMB(model.parameters(), lr=5e-3)
    try:
        opt = FP16_Optimizer(fused, dynamic_loss_scale=True)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            loss = sum(l.sum() for l in model(*args))
            opt.backward(loss)
            opt.step()
            assert opt.overflow is False
            losses.append(loss.item())
        with torch.no_grad():
            losses.append(sum(l.sum() for l in model(*args)).item())
        torch.cuda.synchronize()
        print("FusedLAMB in FP16_Optimizer, tiny model, bf16 mode: losses %s, grad norm %.3f" % (losses, fused.grad_norm.item()))
        assert all(l == l and abs(l) != float("inf") for l in losses), losses
        assert all(b <= a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0], losses
        assert fused.skipped_steps() == 0 and len(fused.trust_ratios) > 20
        assert opt.loss_scale == 1.0 and torch.isfinite(fused.trust_ratios).all()
    finally:
        _native.set_gemm_mode(prev)
        V._drop_p = orig
        _release(fused)
