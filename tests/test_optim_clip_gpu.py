"""Fused global-norm clipping, gradient scale and overflow-safe step of the native AdamW (csrc/optimizer.hip:
grad_sumsq_kernel, grad_norm_finish_kernel, adamw_kernel) on the GPU: norm accuracy, reproducibility, bit-identity with
the plain step where the coefficient is 1 or a power of two, the clipped trajectory against torch.nn.utils.clip_grad_norm_ +
the plain native step, skipped non-finite steps, every construction order of optimizer and DistributedDataParallel, foreign
gradients, and the captured bf16 step. A non-finite gradient here is an ordinary value written with fill_."""
import os
import socket

import pytest
import torch
import torch.distributed as dist

from optim_helpers import DEV, bits_equal as _bits_equal
from optim_helpers import leave_no_workspace_slices_behind  # noqa: F401 (an autouse fixture: the models, wrappers and captured steps of this file bring streams of their own)
from oracle import synth

pytestmark = pytest.mark.gpu
NAMES = ["input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "masked_lm_labels", "image_label", "image_target", "next_sentence_label"]
# sizes of the issue's mixed set; the oddly offset view (data_ptr % 16 == 4, scalar path of every kernel) is added by _params
SIZES = [1, 5, 4097, 3 * 65536 + 3]
ODD = 4099
# tests/test_optim.py::test_native_adamw_matches_the_torch_derived_golden_trajectories: |p - want| <= 3e-6 * max(1, max |want|)
TRAJ_TOL = 3e-6


def _params(seed=3):
    """Parameters of the mixed set (+ the odd view) and a generator for their gradients."""
    g0 = torch.Generator().manual_seed(seed)
    base = torch.randn(ODD + 1, generator=g0).to(DEV)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g0).to(DEV)) for n in SIZES] + [torch.nn.Parameter(base[1:])]
    assert ps[-1].data_ptr() % 16 != 0
    return ps, g0


def _grads(g0, scale=0.1):
    """One gradient per parameter of _params; the last is an odd-offset view like its parameter."""
    gs = [(torch.randn(n, generator=g0) * scale).to(DEV) for n in SIZES]
    gbase = (torch.randn(ODD + 1, generator=g0) * scale).to(DEV)
    assert gbase[1:].data_ptr() % 16 != 0
    return gs + [gbase[1:]]


def _groups(ps):
    return [{"params": ps[:2], "weight_decay": 0.01}, {"params": ps[2:], "weight_decay": 0.0, "lr": 3e-3}]


def _clone_params(ps):
    """Copies at the same 16-byte misalignment (the copy of an odd view takes the scalar path like the original)."""
    out = []
    for p in ps:
        shift = (p.data_ptr() % 16) // 4
        q = torch.empty(p.numel() + shift, device=p.device)[shift:].view(p.shape)
        q.copy_(p.detach())
        assert q.data_ptr() % 16 == p.data_ptr() % 16
        out.append(torch.nn.Parameter(q))
    return out


def _norm64(grads):
    return torch.sqrt(sum((g.double() ** 2).sum() for g in grads)).item()


def _assert_state_bits(opt_a, ps_a, opt_b, ps_b, what):
    for i, (p, q) in enumerate(zip(ps_a, ps_b)):
        assert _bits_equal(p, q), "%s: parameter %d" % (what, i)
        for k in ("exp_avg", "exp_avg_sq"):
            assert _bits_equal(opt_a.state[p][k], opt_b.state[q][k]), "%s: %s of %d" % (what, k, i)


def _assert_trajectory(ps, want, what):
    worst = (0.0, 0.0, -1)
    for i, (p, q) in enumerate(zip(ps, want)):
        err = (p.detach().double() - q.detach().double()).abs().max().item()
        bound = TRAJ_TOL * max(1.0, q.detach().abs().max().item())
        worst = max(worst, (err / bound, err, i))
        assert err <= bound, (what, i, err, bound)
    print("%s: %d tensors, worst max |diff| %.3e = %.3f of its bound (tensor %d)" % (what, len(ps), worst[1], worst[0], worst[2]))


def test_grad_norm_matches_the_float64_norm():
    """Bound 2e-5 relative: the longest fp32 chain of grad_sumsq_kernel is 256 sequential adds (the scalar path of a full
    chunk: CHUNK_ELEMS = 65,536 over 256 threads; the 16-byte path keeps four accumulators of 64 adds each) plus the in-block
    tree (2 + 6 + 2 levels), all on non-negative terms: <= ~266 * 2^-24 = 1.6e-5 on the sum of squares, half of that on the
    norm; the finish kernel adds the per-chunk partials in double."""
    from vilbert.optim import AdamW, CHUNK_ELEMS
    assert CHUNK_ELEMS == 65536
    ps, g0 = _params()
    opt = AdamW(_groups(ps), lr=1e-3, max_grad_norm=1.0)
    for scale in (0.1, 3.0, 1e-4):
        grads = _grads(g0, scale)
        for p, g in zip(ps, grads):
            p.grad = g
        opt.step()
        got, want = opt.grad_norm.item(), _norm64(grads)
        print("grad_norm %.9e, float64 %.9e, relative error %.3e" % (got, want, abs(got - want) / want))
        assert abs(got - want) <= 2e-5 * want
        st = opt._grad_state.cpu()
        assert st[3].item() == 1.0 and st[2].item() == pytest.approx(min(1.0, 1.0 / (want + 1e-6)), rel=3e-5)
    assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda and opt.skipped_steps() == 0


def test_two_norm_passes_on_the_same_gradients_give_the_same_bits():
    from vilbert import _native as N
    from vilbert.optim import AdamW, CHUNK_ELEMS
    ps, g0 = _params(seed=9)
    opt = AdamW(_groups(ps), lr=1e-3, max_grad_norm=0.5)
    grads = _grads(g0)
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()                                   # builds the launch tables (the gradients stay alive in `grads`)
    plan = opt._plan
    out = []
    for _ in range(2):
        partials = torch.full((plan["n_chunks"],), -1.0, device=DEV)
        state = torch.zeros(N.GRAD_STATE_FLOATS, device=DEV)
        N.check(N.lib().vbx_grad_norm(N.stream_ptr(), plan["n_chunks"], plan["dev_tab"].data_ptr(),
                                      plan["chunk_tensor"].data_ptr(), plan["chunk_off"].data_ptr(), CHUNK_ELEMS, 0.5, 1.0, 1,
                                      partials.data_ptr(), state.data_ptr()), "vbx_grad_norm")
        torch.cuda.synchronize()
        out.append((partials, state))
    assert _bits_equal(out[0][0], out[1][0]) and _bits_equal(out[0][1], out[1][1])
    assert (out[0][0] >= 0).all() and out[0][1][N.GRAD_STATE_NORM].item() == pytest.approx(_norm64(grads), rel=2e-5)
    assert _bits_equal(out[0][1][:4], opt._grad_state[:4])      # and the same as the pass inside step()


def test_clipping_above_the_norm_is_bit_identical_to_the_plain_step():
    from vilbert.optim import AdamW
    ps, g0 = _params(seed=5)
    qs = _clone_params(ps)
    plain = AdamW(_groups(ps), lr=1e-2, betas=(0.9, 0.98))
    clipped = AdamW(_groups(qs), lr=1e-2, betas=(0.9, 0.98), max_grad_norm=1e6)
    for _ in range(10):
        grads = _grads(g0)
        for p, q, g in zip(ps, qs, grads):
            p.grad, q.grad = g, g
        plain.step()
        clipped.step()
    torch.cuda.synchronize()
    assert clipped._grad_state[2].item() == 1.0
    _assert_state_bits(plain, ps, clipped, qs, "max_grad_norm above the norm vs plain")


def test_clipped_trajectory_matches_torch_clipping_plus_the_plain_step():
    from vilbert.optim import AdamW
    ps, g0 = _params(seed=6)
    qs = _clone_params(ps)
    max_norm = 1.0
    clipped = AdamW(_groups(ps), lr=1e-2, betas=(0.9, 0.98), max_grad_norm=max_norm)
    plain = AdamW(_groups(qs), lr=1e-2, betas=(0.9, 0.98))
    for step in range(10):
        grads = _grads(g0, scale=0.02 + 0.008 * step)
        ratio = _norm64(grads) / max_norm
        assert 5.0 <= ratio <= 50.0, ratio
        keep = [g.clone() for g in grads]
        for p, q, g in zip(ps, qs, grads):
            p.grad, q.grad = g, g.clone()
        clipped.step()
        torch.nn.utils.clip_grad_norm_(qs, max_norm)
        plain.step()
        for g, k in zip(grads, keep):
            assert _bits_equal(g, k), "step() modified a gradient"
    torch.cuda.synchronize()
    _assert_trajectory(ps, qs, "clipped vs clip_grad_norm_ + plain")


def test_grad_scale_by_a_power_of_two_is_exact():
    from vilbert.optim import AdamW
    ps, g0 = _params(seed=7)
    qs = _clone_params(ps)
    plain = AdamW(_groups(ps), lr=1e-2, weight_decay=0.01)
    scaled = AdamW(_groups(qs), lr=1e-2, weight_decay=0.01, grad_scale=0.125)
    for _ in range(10):
        grads = _grads(g0)
        for p, q, g in zip(ps, qs, grads):
            p.grad, q.grad = g, g * 8.0
        plain.step()
        scaled.step()
    torch.cuda.synchronize()
    _assert_state_bits(plain, ps, scaled, qs, "8 g with grad_scale 1/8 vs g")
    assert scaled._grad_state[2].item() == 0.125


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_step_and_the_next_one_proceeds(bad):
    from vilbert.optim import AdamW
    ps, g0 = _params(seed=8)
    qs = _clone_params(ps)
    kw = dict(lr=1e-2, correct_bias=False, max_grad_norm=1.0)
    opt = AdamW(_groups(ps), skip_nonfinite=True, **kw)
    ref = AdamW(_groups(qs), skip_nonfinite=True, **kw)              # sees the finite steps only
    g1, g2, g3 = _grads(g0), _grads(g0), _grads(g0)
    for p, q, g in zip(ps, qs, g1):
        p.grad, q.grad = g, g
    opt.step()
    ref.step()
    assert opt.skipped_steps() == 0 and not opt.last_step_skipped()
    before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in ps]
    g2[3][65536 + 17].fill_(bad)                   # one element of one gradient
    for p, g in zip(ps, g2):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    for p, (p0, m0, v0) in zip(ps, before):
        assert _bits_equal(p, p0) and _bits_equal(opt.state[p]["exp_avg"], m0) and _bits_equal(opt.state[p]["exp_avg_sq"], v0)
    assert opt.skipped_steps() == 1 and opt.last_step_skipped()
    for p, q, g in zip(ps, qs, g3):
        p.grad, q.grad = g, g
    opt.step()
    ref.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and not opt.last_step_skipped()
    assert all(torch.isfinite(p).all() for p in ps) and not _bits_equal(ps[3], before[3][0])
    _assert_state_bits(ref, qs, opt, ps, "after a skipped step vs the finite steps alone")       # correct_bias=False


@pytest.mark.parametrize("kw", [dict(), dict(grad_scale=0.5)])
def test_without_skip_a_nan_gradient_still_reaches_the_weights(kw):
    """skip_nonfinite=False and max_grad_norm=0: the step runs as it always did and the result has non-finite entries (with
    the defaults that is the plain launch, with a gradient scale the scaled one)."""
    from vilbert.optim import AdamW
    ps, g0 = _params(seed=10)
    opt = AdamW(_groups(ps), lr=1e-2, **kw)
    grads = _grads(g0)
    grads[2][11].fill_(float("nan"))
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    torch.cuda.synchronize()
    assert not torch.isfinite(ps[2]).all() and torch.isfinite(ps[3]).all()
    assert opt.skipped_steps() == 0 and not opt.last_step_skipped()


def test_foreign_gradients_are_counted_and_clipped():
    """One gradient is a slice of the optimizer's arena, the others come from plain torch autograd nodes: all of them are in
    the norm and all of them are clipped."""
    from vilbert import arena as A
    from vilbert.optim import AdamW
    g0 = torch.Generator().manual_seed(12)
    ps = [torch.nn.Parameter(torch.randn(n, generator=g0).to(DEV)) for n in (300, 4097, 70000)]
    qs = _clone_params(ps)
    opt = AdamW(ps, lr=1e-2, max_grad_norm=1.0)
    ref = AdamW(qs, lr=1e-2)
    assert opt._arena is not None and all(A.lookup(p) is not None for p in ps)
    x = [torch.randn(p.shape, generator=g0).to(DEV) for p in ps]
    (ps[1] * x[1]).sum().add((ps[2] * x[2]).sum() * 0.5).backward()          # plain torch nodes: foreign gradients
    i0 = A.lookup(ps[0])[1]
    opt._arena.views[i0].copy_(x[0])
    ps[0].grad = opt._arena.alias(i0)                                         # an arena slice
    assert ps[0].grad.data_ptr() == opt._arena.views[i0].data_ptr()
    assert all(ps[k].grad.data_ptr() != opt._arena.views[A.lookup(ps[k])[1]].data_ptr() for k in (1, 2))
    want = _norm64([p.grad for p in ps])
    assert want > 50.0
    for p, q in zip(ps, qs):
        q.grad = p.grad.clone()
    opt.step()
    torch.nn.utils.clip_grad_norm_(qs, 1.0)
    ref.step()
    torch.cuda.synchronize()
    assert abs(opt.grad_norm.item() - want) <= 2e-5 * want
    _assert_trajectory(ps, qs, "arena slice + foreign gradients")
    opt._arena.release()
    ref._arena.release()


def _model(cfg, sd):
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    m = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
    m.load_state_dict(sd)
    return m.to(DEV).train()


@pytest.fixture
def one_rank_group():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device(DEV))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("order", ["no_ddp", "ddp_before", "ddp_after"])
def test_every_construction_order_clips_like_torch(order, one_rank_group):
    """The real 2-layer / 2-connection model under FP16_Optimizer(FusedAdam(max_grad_norm=1.0)), two steps, with the optimizer
    built without a data-parallel wrapper, after it and BEFORE it (the wrapper's arena then takes the parameters over and the
    optimizer's own arena loses its buffer: the clipping used to crash in vector_norm(None)). Reference: the same gradients
    through torch.nn.utils.clip_grad_norm_ and the plain native step on a copy of the parameters."""
    from apex.optimizers import FP16_Optimizer, FusedAdam
    from vilbert.distributed import DistributedDataParallel as DDP
    from vilbert.optim import AdamW
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "pretraining")
    x = synth.make_inputs(cfg, 8, 20, 37, with_labels=True)
    args = [x[n].to(DEV) for n in NAMES]
    model = _model(cfg, sd)
    kw = dict(lr=1e-4, bias_correction=False, betas=(0.9, 0.98), weight_decay=0.01)
    wrapped = model
    if order == "ddp_before":
        wrapped = DDP(model, message_size=4 * 1024 * 1024)
    fused = FusedAdam(model.parameters(), max_grad_norm=1.0, **kw)
    if order == "ddp_after":
        wrapped = DDP(model, message_size=4 * 1024 * 1024)
        assert fused._arena is not None and fused._arena.flat is None       # taken over by the wrapper's arena
    opt = FP16_Optimizer(fused, dynamic_loss_scale=True)
    params = [p for p in model.parameters()]
    shadow = _clone_params(params)
    ref = AdamW(shadow, lr=kw["lr"], betas=kw["betas"], eps=1e-8, weight_decay=kw["weight_decay"], correct_bias=False)
    if ref._arena is not None:
        ref._arena.release()
    try:
        for step in range(2):
            opt.zero_grad()
            loss = sum(l.sum() for l in wrapped(*args))
            opt.backward(loss)
            torch.cuda.synchronize()
            used = [(p, q) for p, q in zip(params, shadow) if p.grad is not None]
            for p, q in used:
                q.grad = p.grad.detach().clone()
            for p, q in zip(params, shadow):
                if p.grad is None:
                    q.grad = None
            want = _norm64([q.grad for _p, q in used])
            assert want > 1.0, want                                             # the clipping is active
            opt.step()
            torch.nn.utils.clip_grad_norm_([q for _p, q in used], 1.0)
            ref.step()
            assert abs(fused.grad_norm.item() - want) <= 2e-5 * want
            assert opt.overflow is False
        torch.cuda.synchronize()
        _assert_trajectory(params, shadow, order)
        assert len(used) > 100 and fused.skipped_steps() == 0
    finally:
        if wrapped is not model:
            wrapped.arena.release()
        if fused._arena is not None:
            fused._arena.release()


def test_clipped_bf16_step_replays_as_a_graph_like_the_eager_step():
    """set_gemm_mode("bf16"), the 2-layer / 2-connection model, max_grad_norm=1.0: six replays of the captured step against six
    eager steps on the same batch, compared as tests/test_graphed_gpu.py::test_chain_graph_after_freed_memory... compares its
    bf16 case (every loss finite, |eager - replay| <= 3e-2 |eager|); the device-resident norm moves from replay to replay."""
    import vilbert.vilbert as V
    from apex.optimizers import FusedAdam
    from vilbert import _native
    from vilbert.graphed import GraphedTrainStep
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "pretraining")
    orig, V._drop_p = V._drop_p, (lambda m: 0.0)
    prev = _native.set_gemm_mode("bf16")
    try:
        args = [synth.make_inputs(cfg, 4, 12, 10, seed=70, with_labels=True)[k].to(DEV) for k in NAMES]
        m0 = _model(cfg, sd)
        o0 = FusedAdam(m0.parameters(), lr=3e-4, bias_correction=False, eps=1e-6, max_grad_norm=1.0)
        ref, ref_norms = [], []
        for _ in range(6):
            o0.zero_grad()
            loss = sum(l.mean() for l in m0(*args))
            loss.backward()
            o0.step()
            ref.append(loss.item())
            ref_norms.append(o0.grad_norm.item())
        m1 = _model(cfg, sd)
        o1 = FusedAdam(m1.parameters(), lr=3e-4, bias_correction=False, eps=1e-6, max_grad_norm=1.0)
        got, norms = [], []
        with GraphedTrainStep(m1, o1, args, warmup=2, branches="chain") as step:
            for _ in range(6):
                got.append(step(*args).item())
                norms.append(o1.grad_norm.item())
            step.check()
        print("eager losses %s norms %s\nreplay losses %s norms %s" % (ref, ref_norms, got, norms))
        assert all(g == g for g in got), got
        for a, b in zip(ref, got):
            assert abs(a - b) <= 3e-2 * abs(a), (ref, got)
        assert all(n == n and n > 0.0 for n in norms) and len(set(norms)) == 6, norms
        assert max(ref_norms) > 1.0, ref_norms                                 # the clipping was active
        assert o1.skipped_steps() == 0
    finally:
        _native.set_gemm_mode(prev)
        V._drop_p = orig
