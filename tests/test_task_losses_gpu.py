"""GPU side of the native fine-tuning loss and answer score (csrc/task_loss.hip through vilbert/task_losses.py).

The BCE-with-logits loss and its gradient are compared with float64 torch on the SAME fp32 inputs, through the nn.Module
and with an upstream gradient other than 1, at every row width where the kernels change their mapping (n = 256), at sizes
that need one block, several blocks and more partial sums than the finishing block has threads, and on row-strided views.
Tolerances: the loss at rtol 1e-5 / atol 1e-6 (the bar tests/test_kernels_gpu.py sets for the native cross-entropy); the
gradient's elements are ~1 / (rows n), so d * rows * n is compared with (sigmoid(x) - t) * g at the same bar - an absolute
bar on d itself would pass a kernel that writes zeros. The score is compared with upstream's arithmetic on the CPU, bit for
bit. End to end, `ForwardModelsTrain`'s restatement runs through the HIP model with torch's criteria and with the native
ones."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import helpers
from oracle import synth, task_forward_oracle as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 1e-5, 1e-6
UP = 1.7          # the upstream gradient of every backward here

# [rows, n]: one element; the binary / tri heads; one below, at and above the width where rows get a block each; an answer
# head; several blocks of the flat mapping with a ragged tail; more per-row partials (300) than the finishing block has
# threads (256); a [B, R, 1] region logit
BCE_SHAPES = [(1, 1), (3, 2), (5, 3), (4, 255), (4, 256), (4, 257), (6, 3129), (1025, 7), (300, 3129), (7, 101, 1)]


def _close(got, want, what):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    err = (got - want).abs()
    worst = float((err - (ATOL + RTOL * want.abs())).max())
    assert worst <= 0, "%s: max abs err %.3e (max |ref| %.3e)" % (what, float(err.max()), float(want.abs().max()))


def _reference(x, t):
    """float64 loss and d loss / d x * numel (for the upstream gradient UP) on the fp32 values x, t (CPU)."""
    x64, t64 = x.double(), t.double()
    return F.binary_cross_entropy_with_logits(x64, t64, reduction="mean"), (torch.sigmoid(x64) - t64) * UP


def _native_loss_and_grad(x_dev, t_dev):
    from vilbert import task_losses as TL
    loss = TL.BCEWithLogitsLoss(reduction="mean")(x_dev, t_dev)
    assert type(loss.grad_fn).__name__ == "BCEWithLogitsFnBackward", loss.grad_fn          # the native node, not torch's
    (d,) = torch.autograd.grad(loss * UP, x_dev)
    return loss, d


@pytest.mark.parametrize("shape", BCE_SHAPES, ids=["x".join(map(str, s)) for s in BCE_SHAPES])
def test_bce_forward_and_backward_match_float64(shape):
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(*shape, generator=g) * 3
    t = torch.rand(*shape, generator=g) * (torch.rand(*shape, generator=g) < 0.5)          # soft labels, half of them 0
    want_loss, want_d = _reference(x, t)
    xd = x.to(DEV).requires_grad_(True)
    loss, d = _native_loss_and_grad(xd, t.to(DEV))
    assert loss.shape == () and loss.dtype == torch.float32 and d.shape == xd.shape
    _close(loss, want_loss, "loss %s" % (shape,))
    _close(d.cpu().double() * x.numel(), want_d, "gradient %s" % (shape,))


@pytest.mark.parametrize("rows,n,ld", [(37, 1002, 1004), (9, 3, 4)], ids=["37x1002in1004", "9x3in4"])
def test_bce_on_a_row_strided_view_reads_and_writes_the_view_only(rows, n, ld):
    """A head output inside its padded buffer, in both mappings: the padding (NaN) is never read, the gradient comes back
    with the view's row stride and nothing is written between the rows."""
    from vilbert import _native as N
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(rows, n, generator=g) * 3, torch.rand(rows, n, generator=g)
    want_loss, want_d = _reference(x, t)
    buf = torch.full((rows, ld), float("nan"), device=DEV)
    tbuf = torch.full((rows, ld + 4), float("nan"), device=DEV)
    buf[:, :n] = x.to(DEV)
    tbuf[:, :n] = t.to(DEV)
    xv = buf[:, :n].requires_grad_(True)
    loss, d = _native_loss_and_grad(xv, tbuf[:, :n])
    assert d.shape == (rows, n) and d.stride() == (ld, 1)
    _close(loss, want_loss, "loss of the view")
    _close(d.cpu().double() * (rows * n), want_d, "gradient of the view")
    assert torch.isnan(buf[:, n:]).all() and torch.isnan(tbuf[:, n:]).all()
    # the C entry point on a pre-filled output: the same bits inside the view, the padding keeps its content
    out = torch.full((rows, ld), 7.0, device=DEV)
    up = torch.full((1,), UP, device=DEV)
    N.check(N.lib().vbt_bce_bwd(N.stream_ptr(), rows, n, buf.data_ptr(), ld, tbuf.data_ptr(), ld + 4, up.data_ptr(),
                                out.data_ptr(), ld), "vbt_bce_bwd")
    torch.cuda.synchronize()
    assert torch.equal(out[:, :n], d) and (out[:, n:] == 7.0).all()


def test_bce_is_stable_at_large_logits():
    x = torch.tensor([90.0, -90.0, 20.0, -20.0, 0.0]).repeat_interleave(3).view(5, 3)
    t = torch.tensor([0.0, 1.0, 0.3]).repeat(5).view(5, 3)
    want_loss, want_d = _reference(x, t)
    assert float(want_loss) > 20.0                 # the +-90 entries against the far label contribute 90 each
    loss, d = _native_loss_and_grad(x.to(DEV).requires_grad_(True), t.to(DEV))
    assert torch.isfinite(loss).all() and not torch.isnan(d).any()
    _close(loss, want_loss, "loss at +-90")
    _close(d.cpu().double() * x.numel(), want_d, "gradient at +-90")
    # |x| = 100 (the bound the backward is specified for) in the block-per-row mapping
    x = torch.tensor([100.0, -100.0]).repeat(2, 150)
    t = torch.tensor([0.0, 0.0, 1.0, 1.0]).repeat(2, 75)
    want_loss, want_d = _reference(x, t)
    loss, d = _native_loss_and_grad(x.to(DEV).requires_grad_(True), t.to(DEV))
    _close(loss, want_loss, "loss at +-100")
    _close(d.cpu().double() * x.numel(), want_d, "gradient at +-100")


@pytest.mark.parametrize("shape", [(300, 3129), (1025, 7)], ids=["300x3129", "1025x7"])
def test_bce_is_bit_identical_from_call_to_call(shape):
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(*shape, generator=g) * 3).to(DEV).requires_grad_(True)
    t = torch.rand(*shape, generator=g).to(DEV)
    loss1, d1 = _native_loss_and_grad(x, t)
    loss2, d2 = _native_loss_and_grad(x, t)
    assert torch.equal(loss1, loss2) and torch.equal(d1, d2)


def _upstream_score(logits, labels):
    """compute_score_with_logits as upstream writes it (task_utils.py:618-623), on the CPU."""
    logits = torch.max(logits, 1)[1].data
    one_hots = torch.zeros(*labels.size())
    one_hots.scatter_(1, logits.view(-1, 1), 1)
    return one_hots * labels


SCORE_SHAPES = [(6, 3129), (5, 3), (9, 2), (7, 101, 1)]


@pytest.mark.parametrize("shape", SCORE_SHAPES, ids=["x".join(map(str, s)) for s in SCORE_SHAPES])
def test_scores_match_upstreams_arithmetic(shape):
    from vilbert import task_losses as TL
    g = torch.Generator().manual_seed(3 + sum(shape))
    logits, labels = torch.randn(*shape, generator=g), torch.rand(*shape, generator=g)
    l2, t2 = (logits.squeeze(2), labels.squeeze(2)) if len(shape) == 3 else (logits, labels)
    top = l2.topk(2, dim=1).values
    assert ((top[:, 0] - top[:, 1]) > 0).all()          # precondition: no ties, the arg-max is unambiguous
    want_idx = torch.max(l2, 1)[1]
    want_picked = t2.gather(1, want_idx.view(-1, 1)).view(-1)
    idx, picked = TL.row_argmax_pick(logits.to(DEV), labels.to(DEV))
    assert idx.dtype == torch.int64 and picked.dtype == torch.float32
    assert torch.equal(idx.cpu(), want_idx) and torch.equal(picked.cpu(), want_picked)
    dense = TL.compute_score_with_logits(logits.to(DEV), labels.to(DEV))
    assert dense.shape == labels.shape and dense.dtype == torch.float32 and dense.is_cuda
    assert torch.equal(dense.cpu().view(t2.shape), _upstream_score(l2, t2))
    assert int((dense != 0).sum()) <= shape[0]
    if len(shape) == 2:          # the same rows inside NaN-padded buffers: the row strides are honoured, the padding is not read
        lbuf, tbuf = (torch.full((shape[0], shape[1] + 3), float("nan"), device=DEV) for _ in range(2))
        lbuf[:, :shape[1]] = logits.to(DEV)
        tbuf[:, :shape[1]] = labels.to(DEV)
        idx, picked = TL.row_argmax_pick(lbuf[:, :shape[1]], tbuf[:, :shape[1]])
        assert torch.equal(idx.cpu(), want_idx) and torch.equal(picked.cpu(), want_picked)
        assert torch.equal(TL.compute_score_with_logits(lbuf[:, :shape[1]], tbuf[:, :shape[1]]), dense)


@pytest.mark.parametrize("n", [3, 3129])
def test_scores_on_ties_and_nan(n):
    from vilbert import task_losses as TL
    g = torch.Generator().manual_seed(n)
    logits, labels = torch.randn(4, n, generator=g), torch.rand(4, n, generator=g) + 0.25
    hi = n - 1
    logits[0, hi] = logits[0, 1] = 50.0                 # a tie: the lowest index wins
    logits[1, :] = -float("inf")                        # every element ties
    logits[2, hi] = float("nan")                        # a NaN counts as the maximum ...
    logits[2, 0] = 60.0
    logits[3, 2 % n] = 70.0
    want = torch.max(logits, 1)[1]
    assert want.tolist() == [1, 0, hi, 2 % n]           # ... in torch's order too
    idx, picked = TL.row_argmax_pick(logits.to(DEV), labels.to(DEV))
    assert idx.cpu().tolist() == want.tolist()
    assert torch.equal(picked.cpu(), labels[torch.arange(4), want])
    dense = TL.compute_score_with_logits(logits.to(DEV), labels.to(DEV))
    assert torch.equal(dense.cpu(), _upstream_score(logits, labels))


def test_everything_else_falls_back_to_torch():
    from vilbert import task_losses as TL
    g = torch.Generator().manual_seed(2)
    x, t = torch.randn(6, 10, generator=g).to(DEV), torch.rand(6, 10, generator=g).to(DEV)
    pw = (torch.rand(10, generator=g) + 0.5).to(DEV)
    for kwargs, xx, tt in ((dict(reduction="sum"), x, t), (dict(reduction="none"), x, t), (dict(pos_weight=pw), x, t),
                           (dict(weight=pw), x, t), (dict(), x.bfloat16(), t.bfloat16()), (dict(), x.double(), t.double())):
        a = xx.clone().requires_grad_(True)
        b = xx.clone().requires_grad_(True)
        got, want = TL.BCEWithLogitsLoss(**kwargs)(a, tt), nn.BCEWithLogitsLoss(**kwargs)(b, tt)
        assert "BCEWithLogitsFn" not in type(got.grad_fn).__name__
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), kwargs
        got.sum().backward()
        want.sum().backward()
        assert a.grad.dtype == xx.dtype and torch.equal(a.grad, b.grad), kwargs
    # a target that wants a gradient gets torch's
    a, tg = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
    TL.BCEWithLogitsLoss()(a, tg).backward()
    assert tg.grad is not None
    # cross-entropy: the plain case is the native node, class weights / label smoothing / probabilities are torch's
    y = torch.tensor([0, 3, 9, -100, 2, 2], device=DEV)
    a, b = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    got, want = TL.CrossEntropyLoss()(a, y), nn.CrossEntropyLoss()(b, y)
    assert type(got.grad_fn).__name__ == "CrossEntropyFnBackward"
    (got * UP).backward()
    (want * UP).backward()
    assert torch.allclose(got, want, rtol=1e-5, atol=1e-6) and torch.allclose(a.grad, b.grad, rtol=1e-5, atol=1e-7)
    for kwargs in (dict(weight=pw), dict(label_smoothing=0.1), dict(reduction="sum")):
        got, want = TL.CrossEntropyLoss(**kwargs)(a, y), nn.CrossEntropyLoss(**kwargs)(b, y)
        assert "CrossEntropyFn" not in type(got.grad_fn).__name__ and torch.equal(got, want), kwargs
    # scores of tensors the kernel does not take: upstream's arithmetic and upstream's dtype (its one-hot matrix is fp32, so
    # the product with bf16 labels promotes to fp32)
    lb, tb = x.bfloat16(), t.bfloat16()
    got = TL.compute_score_with_logits(lb, tb)
    want = _upstream_score(lb.cpu(), tb.cpu())
    assert got.is_cuda and got.dtype == want.dtype == torch.float32 and torch.equal(got.cpu(), want)


def test_bce_forward_and_backward_replay_from_a_hip_graph():
    from vilbert import task_losses as TL
    crit = TL.BCEWithLogitsLoss(reduction="mean")
    g = torch.Generator().manual_seed(17)
    shape = (130, 3129)
    t = torch.rand(*shape, generator=g).to(DEV)
    static_x = (torch.randn(*shape, generator=g) * 2).to(DEV).requires_grad_(True)

    def step():
        loss = crit(static_x, t)
        (d,) = torch.autograd.grad(loss * UP, static_x)
        return loss, d
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                          # warm-up on a side stream, the documented capture pattern
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        cap_loss, cap_d = step()
    first_loss, first_d = step()
    first_loss, first_d = first_loss.clone(), first_d.clone()
    with torch.no_grad():
        static_x.copy_((torch.randn(*shape, generator=g) * 2).to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    got_loss, got_d = cap_loss.clone(), cap_d.clone()
    want_loss, want_d = step()
    assert torch.equal(got_loss, want_loss) and torch.equal(got_d, want_d)
    assert not torch.equal(got_loss, first_loss) and not torch.equal(got_d, first_d)          # the input did change


# task, batch, tokens, regions, task_specific_tokens: the cases of tests/test_task_forward_gpu.py for the four head types
E2E_CASES = [("TASK1", 6, 23, 101, True), ("TASK4", 4, 20, 200, True), ("TASK8", 2, 30, 101, False),
             ("TASK12", 4, 40, 101, True)]


@pytest.mark.parametrize("task_id,batch,n_tok,n_reg,task_tokens", E2E_CASES, ids=[c[0] for c in E2E_CASES])
def test_forward_models_train_with_the_native_criteria_matches_torchs(task_id, batch, n_tok, n_reg, task_tokens, monkeypatch):
    """The model, state dict and batch of tests/test_task_forward_gpu.py; `forward_train` through the HIP model with
    torch's criteria and score, then with the native ones: equal score, loss within 1e-5 relative, every parameter gradient
    within the bound that file sets between the HIP model and the oracle."""
    import vilbert.vilbert as V
    from vilbert import task_losses as TL
    from vilbert.vilbert import BertConfig, VILBertForVLTasks

    cfg = synth.load_config("bert_base_2layer_2conect.json")
    cfg.update(v_target_size=1601, task_specific_tokens=task_tokens)
    sd = synth.make_state_dict(cfg, "vltasks", seed=21)
    data = helpers.to_device(tf.make_task_batch(task_id, batch, n_tok, n_reg, num_labels=3129, seed=31), DEV)
    monkeypatch.setattr(V, "_drop_p", lambda m: 0.0)
    net = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=3129)
    net.load_state_dict(sd)
    net = net.to(DEV).train()

    def run():
        net.zero_grad(set_to_none=True)
        loss, score = tf.forward_train(task_id, data, net)
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), float(score), {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    want_loss, want_score, want_grads = run()
    monkeypatch.setattr(tf, "LOSSES", {"BCEWithLogitLoss": TL.BCEWithLogitsLoss(reduction="mean"),
                                       "CrossEntropyLoss": TL.CrossEntropyLoss()})
    monkeypatch.setattr(tf, "score_with_logits", TL.compute_score_with_logits)
    got_loss, got_score, got_grads = run()

    assert got_score == want_score
    assert abs(got_loss - want_loss) <= 1e-5 * abs(want_loss), (got_loss, want_loss)
    assert sorted(got_grads) == sorted(want_grads)
    gmax = max(v.abs().max().item() for v in want_grads.values())
    seen = 0
    for name, ref in want_grads.items():
        err = (got_grads[name].double() - ref.double()).abs().max().item()
        bound = 2e-4 * ref.abs().max().item() + 2e-7 * gmax + 5e-7
        assert err <= bound, "%s %s: grad err %.3e > %.3e" % (task_id, name, err, bound)
        seen += 1
    assert seen > 100
