"""The native single-stream baseline model (vilbert/basebert.py) against outputs and gradients recorded from the REAL reference
(tests/golden/make_basebert_golden.py; weights and inputs regenerated from the seeds of tests/basebert_synth.py): forward parity
of the seven heads on the tiny model and on the base config at the task shape (38 + 101 = 139 keys), the bf16x6 GEMM mode,
every parameter gradient with the padding rows of the four padding_idx tables, training mode with dropout, head selection and
one HIP-graph replay of a training step."""
import json

import numpy as np
import pytest
import torch

import basebert_synth as BS
import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_GOLDEN = {}


def _golden(case):
    if case not in _GOLDEN:
        with np.load(BS.path(case)) as z:
            _GOLDEN[case] = {k: z[k] for k in z.files}
    return _GOLDEN[case]


def _model(case, train=False):
    from vilbert.basebert import BaseBertForVLTasks
    torch.manual_seed(0)
    model = BaseBertForVLTasks(BS.config(case), num_labels=BS.CASES[case]["num_labels"])
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(BS.make_state_dict(shapes))
    model = model.to(DEV)
    return model.train() if train else model.eval()


def _args(case, seed=11):
    x = BS.make_inputs(case, seed=seed)
    return x, helpers.to_device(BS.forward_args(x), DEV)


def _check_forward(case):
    model = _model(case)
    _, args = _args(case)
    with torch.no_grad():
        outs = model(*args)
    assert len(outs) == 7
    gold = _golden(case)
    for name, o in zip(BS.HEADS, outs):
        err = helpers.assert_close(BS.sample(case, name, o), gold[name], "%s %s" % (case, name))
        print("%s %-22s %-18s max abs err %.3e" % (case, name, tuple(o.shape), err))
    return outs


@pytest.mark.parametrize("case", ["basebert_tiny", "basebert_base_2l"])
def test_forward_matches_the_reference(case):
    outs = _check_forward(case)
    c = BS.CASES[case]
    B, T, R = c["batch"], c["n_tok"], c["n_reg"]
    vocab = c["cfg"]()["vocab_size"]
    assert [tuple(o.shape) for o in outs] == [(B, c["num_labels"]), (B, 1), (B, 2), (B, R, 1601), (B, R, 1), (B, T, vocab),
                                              (B, T, 1)]


def test_forward_in_the_bf16x6_gemm_mode():
    from vilbert import _native
    prev = _native.set_gemm_mode("bf16x6")
    try:
        _check_forward("basebert_tiny")
    finally:
        _native.set_gemm_mode(prev)


def test_forward_refuses_the_bf16_fp8_and_mx_modes_up_front():
    from vilbert import _native
    model = _model("basebert_tiny")
    _, args = _args("basebert_tiny")
    for mode in ("bf16", "fp8", "mxfp8"):
        prev = _native.set_gemm_mode(mode)
        try:
            with pytest.raises(NotImplementedError, match="fp32 stream only"):
                model(*args)
        finally:
            _native.set_gemm_mode(prev)
    with torch.no_grad():
        model(*args)


def test_bert_model_returns_the_layers_and_the_pooled_output():
    model = _model("basebert_tiny").bert
    _, args = _args("basebert_tiny")
    with torch.no_grad():
        layers, pooled = model(*args)                                      # default: all encoded layers, as the reference
        last, pooled2 = model(*args, output_all_encoded_layers=False)
    assert isinstance(layers, list) and len(layers) == 2 and torch.is_tensor(last)
    assert torch.equal(layers[-1], last) and torch.equal(pooled, pooled2)
    assert tuple(last.shape) == (3, 12, 64) and tuple(pooled.shape) == (3, 64)
    assert float(pooled.abs().max()) <= 1.0


def test_gradients_match_the_reference_and_the_padding_rows_get_none():
    """Eval mode with autograd on (the reference's own backward raises in train mode). Bound per tensor, over the pinned
    positions: |got - ref| <= 2e-4 max|ref| + 2e-7 gmax, the project's gradient criterion
    (tests/test_backward_gpu.py::_grad_parity)."""
    case = "basebert_tiny"
    model = _model(case)
    x, args = _args(case)
    BS.weighted_loss(model(*args), x["image_attention_mask"].to(DEV)).backward()
    gold = _golden(case)
    index = json.loads(str(gold["grad_index"]))
    values = gold["grad_values"]
    named = dict(model.named_parameters())
    assert sorted(index) == sorted(named)
    gmax = max(e["absmax"] for e in index.values())
    worst = 0.0
    for name, e in index.items():
        g = named[name].grad
        assert g is not None and list(g.shape) == e["shape"], name
        got = g.detach().cpu().numpy().reshape(-1)[::e["stride"]].astype(np.float64)
        ref = values[e["offset"]:e["offset"] + e["size"]].astype(np.float64)
        err = float(np.abs(got - ref).max()) if got.size else 0.0
        bound = 2e-4 * e["absmax"] + 2e-7 * gmax
        worst = max(worst, err / bound)
        assert err <= bound, "%s: grad err %.3e > bound %.3e (max|ref| %.3e, model max %.3e)" % (name, err, bound, e["absmax"], gmax)
    print("basebert_tiny gradients: worst err / bound %.3f over %d tensors" % (worst, len(index)))
    rows0 = [named[n].grad[0].cpu() for n in BS.PADDED_TABLES]
    for i in (1, 2, 3):                                                    # position, text token-type, image token-type
        assert float(np.abs(gold["grad_row0_%d" % i]).max()) == 0.0
        assert float(rows0[i].abs().max()) == 0.0, BS.PADDED_TABLES[i]
    ref0 = torch.from_numpy(gold["grad_row0_0"])                           # word row 0: the tied decoder's gradient
    assert float(ref0.abs().max()) > 0.0 and float(rows0[0].abs().max()) > 0.0
    e = index[BS.PADDED_TABLES[0]]
    assert float((rows0[0] - ref0).abs().max()) <= 2e-4 * e["absmax"] + 2e-7 * gmax


def _reseed(seed):
    """torch.manual_seed and the per-process call counter the dropout seeds are mixed from (autograd_ops.next_seed)."""
    import itertools
    from vilbert import autograd_ops as AO
    torch.manual_seed(seed)
    AO._seed_counter = itertools.count(1)


def _train_grads(model, batches):
    model.zero_grad(set_to_none=True)
    losses = []
    for x, args in batches:
        loss = BS.weighted_loss(model(*args), x["image_attention_mask"].to(DEV))
        loss.backward()
        losses.append(loss.item())
    return losses, {n: p.grad.clone() for n, p in model.named_parameters()}


def test_training_mode_with_dropout_is_seeded_and_micro_batches_accumulate():
    case = "basebert_tiny"
    model = _model(case, train=True)
    b1, b2 = _args(case, seed=11), _args(case, seed=12)
    _reseed(5)
    l1, g1 = _train_grads(model, [b1])
    _reseed(5)
    l1b, g1b = _train_grads(model, [b1])
    _reseed(6)
    l1c, _ = _train_grads(model, [b1])
    assert np.isfinite(l1).all() and l1 == l1b and l1 != l1c
    for n in g1:
        assert torch.equal(g1[n], g1b[n]), n
    eval_loss = BS.weighted_loss(model.eval()(*b1[1]), b1[0]["image_attention_mask"].to(DEV)).item()
    model.train()
    assert eval_loss != l1[0]
    # two accumulated micro-batches: the sum of their gradients. Without dropout, so that the two passes are the same
    # functions as the single ones (the masks are drawn from a per-call counter)
    import vilbert.vilbert as V
    import vilbert.basebert as Bb
    orig_v, orig_b = V._drop_p, Bb._drop_p
    V._drop_p = Bb._drop_p = lambda m: 0.0
    try:
        _, ga = _train_grads(model, [b1])
        _, gb = _train_grads(model, [b2])
        _, gab = _train_grads(model, [b1, b2])
    finally:
        V._drop_p, Bb._drop_p = orig_v, orig_b
    gmax = max(float(g.abs().max()) for g in gab.values())
    for n in gab:
        want = ga[n].double() + gb[n].double()
        err = float((gab[n].double() - want).abs().max())
        assert err <= 2e-5 * float(want.abs().max()) + 1e-6 * gmax, n
    for n in BS.PADDED_TABLES[1:]:
        assert float(gab[n][0].abs().max()) == 0.0, n


def test_micro_batches_accumulate_in_the_gradient_arena_too():
    """With an optimizer the gradients are arena slices and the second pass adds in place (also the image token-type row and
    the location projection, which the joint embedding node adds itself)."""
    from vilbert.optim import AdamW
    case = "basebert_tiny"
    b1, b2 = _args(case, seed=11), _args(case, seed=12)
    plain = _model(case)
    _, ga = _train_grads(plain, [b1])
    _, gb = _train_grads(plain, [b2])
    model = _model(case)
    opt = AdamW(model.parameters(), lr=0.0)
    _, gab = _train_grads(model, [b1, b2])
    gmax = max(float(g.abs().max()) for g in gab.values())
    for n in gab:
        want = ga[n].double() + gb[n].double()
        assert float((gab[n].double() - want).abs().max()) <= 2e-5 * float(want.abs().max()) + 1e-6 * gmax, n
    for n in BS.PADDED_TABLES[1:]:
        assert float(gab[n][0].abs().max()) == 0.0, n
    del opt


def test_selected_heads_are_bit_equal_and_the_others_launch_nothing():
    case = "basebert_tiny"
    model = _model(case)
    _, args = _args(case)
    with torch.no_grad():
        full = model(*args)
        model.set_active_heads(["vil_prediction"])
        one = model(*args)
        model.set_active_heads(["vision_logit", "linguisic_prediction"])
        two = model(*args)
        model.set_active_heads(None)
    assert [o is None for o in one] == [False] + [True] * 6
    assert torch.equal(one[0], full[0])
    assert [o is None for o in two] == [True, True, True, True, False, False, True]
    assert torch.equal(two[4], full[4]) and torch.equal(two[5], full[5])


def test_one_graph_replay_of_a_training_step_gives_the_eager_loss():
    import vilbert.basebert as Bb
    import vilbert.vilbert as V
    from vilbert.graphed import GraphedTrainStep
    from vilbert.optim import AdamW
    case = "basebert_tiny"
    _, args = _args(case)
    labels = torch.randint(0, 13, (3,), generator=torch.Generator().manual_seed(2)).to(DEV)
    onehot = torch.nn.functional.one_hot(labels, 13).float()

    def loss_fn(outs):
        return ((outs[0] - onehot) ** 2).mean()

    orig_v, orig_b = V._drop_p, Bb._drop_p
    V._drop_p = Bb._drop_p = lambda m: 0.0
    try:
        m0 = _model(case, train=True)
        m0.set_active_heads(["vil_prediction"])
        o0 = AdamW(m0.parameters(), lr=1e-3, weight_decay=0.01)
        o0.zero_grad()
        eager = loss_fn(m0(*args))
        eager.backward()
        o0.step()
        m1 = _model(case, train=True)
        m1.set_active_heads(["vil_prediction"])
        o1 = AdamW(m1.parameters(), lr=1e-3, weight_decay=0.01)
        with GraphedTrainStep(m1, o1, args, loss_fn=loss_fn, warmup=2) as step:
            got = step(*args).item()
            step.check()
        assert got == pytest.approx(eager.item(), rel=2e-4), (got, eager.item())
        for (n, p), (_, q) in zip(m0.named_parameters(), m1.named_parameters()):
            assert torch.allclose(p, q, rtol=2e-3, atol=2e-5), n
    finally:
        V._drop_p, Bb._drop_p = orig_v, orig_b
