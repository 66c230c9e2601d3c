"""Output + feed-forward block of the last encoder layers on the rows the losses read (csrc/layers.hip vb_ffn_block.row_map,
csrc/rowmap.hip, vilbert/layers.py SelfLayerFn(rows), vilbert.BertForMultiModalPreTraining.forward).

The rows a pre-training step reads from the layers behind the last connection layer are row 0 of every sample and the labelled
rows; everything else those layers' output + FFN blocks compute is discarded in forward and contributes exact zeros in
backward. Running the forward and the input-gradient chain of the block on those rows alone (the reductions over rows stay at
full size, on zero-expanded operands) must therefore change nothing but, at most, the GEMM configuration at the smaller M - in
particular the dropout masks must be those of the whole step (a different mask moves losses and gradients by orders of
magnitude more than the bounds below).
Bounds: those of tests/test_graphed_gpu.py::test_static_capacity_losses_and_gradients_equal_the_exact_gather for a reordering
of this size - losses rel 1e-5, gradients 2e-5 x max + 1e-6 x global max."""
import itertools

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "masked_lm_labels", "image_label", "image_target", "next_sentence_label"]


def _close(got, want, gmax, what):
    err = (got - want).abs().max().item()
    if err > 0.0:
        print("%s: max diff %.3e (max %.3e)" % (what, err, want.abs().max().item()))
    assert err <= 2e-5 * want.abs().max().item() + 1e-6 * gmax, "%s: max diff %.3e" % (what, err)


def test_block_on_a_row_map_equals_the_whole_block_at_the_mapped_rows(monkeypatch):
    """One BertLayer through vb_layer_fwd / vb_layer_bwd, dropout ON, B = 3 samples of 5 tokens, one head of 32 (the smallest
    the launcher takes). The map holds the three pooler rows, three more rows and one padding entry; row 0 is pooler row AND
    labelled row: it is in the map once and has two readers. Against the same layer without a map: y at the mapped rows, dx
    of every row, every parameter gradient; the expanded d_ctx / d_sum1 the attention block reads are exactly zero at the
    rows no entry names."""
    import vilbert.autograd_ops as AO
    from vilbert import layers
    from vilbert.vilbert import BertConfig, BertLayer
    B, S, H = 3, 5, 32
    cfg = synth.tiny_config(hidden_size=H, num_attention_heads=1, intermediate_size=40)
    torch.manual_seed(7)
    layer = BertLayer(BertConfig.from_dict(cfg)).to(DEV).train()
    for p in layer.parameters():                      # (biases and LayerNorm parameters away from their 0 / 1 defaults)
        p.data.add_(torch.randn_like(p) * 0.05)
    x0 = torch.randn(B, S, H, device=DEV)
    mask = torch.zeros(B, 1, 1, S, device=DEV)
    mask[1, 0, 0, 4] = -10000.0
    rows = torch.tensor([0, 5, 10, 7, -1, 13, 2], dtype=torch.int32, device=DEV)
    valid = rows >= 0
    src = rows.to(torch.int64).clamp(min=0)
    w = torch.randn(rows.numel(), H, device=DEV) * valid.unsqueeze(1)        # (a padding row never gets a gradient)
    w0 = torch.randn(H, device=DEV)                                          # the second reader of row 0

    allocs = []
    alloc0 = layers._Carver.alloc
    monkeypatch.setattr(layers._Carver, "alloc", lambda self, device: allocs.append((self, alloc0(self, device))) or allocs[-1][1])

    def run(row_map):
        AO._seed_counter = itertools.count(1)
        x = x0.clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        del allocs[:]
        y = layers.self_layer(layer, x, mask, 0.1, 0.1, 0.1, row_map)
        assert y is not None
        picked = y if row_map is not None else y.reshape(-1, H).index_select(0, src)
        ((picked * w).sum() + (picked[0] * w0).sum()).backward()
        torch.cuda.synchronize()
        return picked.detach() * valid.unsqueeze(1), x.grad.clone(), {n: p.grad.clone() for n, p in layer.named_parameters()}

    y_all, dx_all, g_all = run(None)
    y_map, dx_map, g_map = run(rows)
    assert y_map.shape == (rows.numel(), H) and not y_map[4].any()
    gmax = max(g.abs().max().item() for g in g_all.values())
    _close(y_map, y_all, 0.0, "y")
    _close(dx_map, dx_all, gmax, "dx")
    assert set(g_map) == set(g_all) and len(g_all) == 16
    for n, g in g_all.items():
        _close(g_map[n], g, gmax, n)

    # the full-size gradients the block handed to the attention block (temporaries of the backward call)
    plan = [e for e in layers._PLANS[layer].values()][0][1]["rows"]
    tbuf = [t for c, t in allocs if c is plan.c_bwd][0]
    named = set(src[valid].tolist())
    unnamed = torch.tensor([r for r in range(B * S) if r not in named], device=DEV)
    for name in ("d_ctx", "d_sum1"):
        off = plan.c_bwd.off[name]
        full = tbuf[off:off + B * S * H * 4].view(torch.float32).view(B * S, H)
        assert not full[unnamed].any(), name
        assert full[torch.tensor(sorted(named), device=DEV)].abs().sum(1).min().item() > 0.0, name


def _train_step(cfg, sd, args, capacity=0.5):
    import vilbert.autograd_ops as AO
    from vilbert import layers
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    m = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    m.label_capacity = capacity
    AO._seed_counter = itertools.count(1)
    out = m(*args)
    sum(l.sum() for l in out).backward()
    m.check_label_capacity()
    torch.cuda.synchronize()
    enc = m.bert.encoder
    pruned = ["rows" in ent[1] for last in (enc.layer[-1], enc.v_layer[-1]) for ent in layers._PLANS.get(last, {}).values()]
    return [l.item() for l in out], {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}, pruned


@pytest.mark.parametrize("config,shape", [("bert_base_2layer_2conect.json", (4, 9, 7)), (None, (6, 9, 8))])
def test_pretraining_step_equals_the_step_on_every_row_dropout_on(config, shape, monkeypatch):
    from vilbert import _native
    cfg = synth.load_config(config) if config else synth.tiny_config()
    sd = synth.make_state_dict(cfg, "pretraining")
    args = [synth.make_inputs(cfg, *shape, seed=40, with_labels=True)[n].to(DEV) for n in NAMES]
    assert (args[6][:, 0] != -1).any(), "the batch should label a token 0 (pooler row and labelled row at once)"
    prev = _native.set_gemm_mode("f32")
    try:
        monkeypatch.setenv("VB_LAST_LAYER_ROWS", "0")
        l_all, g_all, pruned = _train_step(cfg, sd, args)
        assert pruned == [False, False]
        monkeypatch.delenv("VB_LAST_LAYER_ROWS")
        l_rows, g_rows, pruned = _train_step(cfg, sd, args)
        assert pruned == [True, True]
    finally:
        _native.set_gemm_mode(prev)
    print("losses on every row %r, on the needed rows %r" % (l_all, l_rows))
    assert l_rows == pytest.approx(l_all, rel=1e-5)
    assert g_rows.keys() == g_all.keys()
    gmax = max(g.abs().max().item() for g in g_all.values())
    for n, g in g_all.items():
        _close(g_rows[n], g, gmax, n)


def test_the_exact_gather_and_inference_keep_every_row():
    from vilbert import layers
    cfg = synth.tiny_config()
    sd = synth.make_state_dict(cfg, "pretraining")
    args = [synth.make_inputs(cfg, 6, 9, 8, seed=40, with_labels=True)[n].to(DEV) for n in NAMES]
    assert _train_step(cfg, sd, args, capacity=None)[2] == [False, False]
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    m = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
    m.load_state_dict(sd)
    m = m.to(DEV).eval()
    m.label_capacity = 0.5
    with torch.no_grad():
        out = m(*args)
    assert all(torch.isfinite(l).all() for l in out)
    assert not any("rows" in ent[1] for ent in layers._PLANS.get(m.bert.encoder.layer[-1], {}).values())


def test_graphed_step_with_the_row_maps_trains_like_the_eager_step():
    """HIP-graph replay with the row maps active (GraphedTrainStep fixes the gather capacity, so the captured step runs the
    last layers on the needed rows) against the eager step at the same capacity; bound: tests/test_graphed_gpu.py."""
    import vilbert.vilbert as V
    from vilbert import layers
    from vilbert.graphed import GraphedTrainStep
    from vilbert.optim import AdamW
    cfg = synth.tiny_config()
    sd = synth.make_state_dict(cfg, "pretraining")
    data = [[synth.make_inputs(cfg, 6, 9, 8, seed=40 + i, with_labels=True)[k].to(DEV) for k in NAMES] for i in range(3)]

    def model():
        m = V.BertForMultiModalPreTraining(V.BertConfig.from_dict(cfg))
        m.load_state_dict(sd)
        return m.to(DEV).train()

    orig, V._drop_p = V._drop_p, (lambda m: 0.0)
    try:
        m0 = model()
        m0.label_capacity = 0.25
        o0 = AdamW(m0.parameters(), lr=1e-3, weight_decay=0.01)
        want = []
        for args in data:
            o0.zero_grad()
            loss = sum(l.mean() for l in m0(*args))
            loss.backward()
            o0.step()
            want.append(loss.item())
        m1 = model()
        o1 = AdamW(m1.parameters(), lr=1e-3, weight_decay=0.01)
        with GraphedTrainStep(m1, o1, data[0], label_capacity=0.25, warmup=2) as step:
            got = [step(*args).item() for args in data]
            step.check()
        for m in (m0, m1):
            assert all("rows" in ent[1] for ent in layers._PLANS[m.bert.encoder.layer[-1]].values())
        assert got == pytest.approx(want, rel=2e-4), (got, want)
    finally:
        V._drop_p = orig
