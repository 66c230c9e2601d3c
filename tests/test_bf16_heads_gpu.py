"""bf16 training mode, model level: poolers, prediction heads and losses on the bf16 stream
(BertForMultiModalPreTraining._losses_on_the_bf16_stream; csrc/heads16.hip; tests/test_heads16_gpu.py holds the kernels).

  * launch census: behind the encoder only the 2-wide alignment head still is an fp32-tensor linear, and no cast sees a
    whole hidden state;
  * parity with the fp32 CPU oracle at the bars of tests/test_bf16_stream_gpu.py (2-layer config), and per head tensor
    against the path this one replaces (VB_BF16_HEADS=0), same inputs: at most 1.5 x its error;
  * the exact and the fixed-capacity label gather agree up to the regrouping of fp32 sums;
  * VB_BF16_HEADS=0 (child process) restores the fp32-tensor launches;
  * a captured step refreshes the zero-padded decoder shadow from the live weights and trains like its eager twin."""
import os
import subprocess
import sys

import pytest
import torch

import helpers
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "masked_lm_labels", "image_label", "image_target", "next_sentence_label")
B, T, R = 4, 36, 37
# the tensors whose gradient the new path computes differently (the transform activations are rounded to bf16 once more)
HEAD_TENSORS = ("bert.t_pooler.dense.", "bert.v_pooler.dense.", "cls.predictions.transform.", "cls.imagePredictions.transform.",
                "cls.predictions.bias", "cls.imagePredictions.decoder.", "bert.embeddings.word_embeddings.weight")


@pytest.fixture
def bf16_mode():
    from vilbert import _native
    prev = _native.set_gemm_mode("bf16")
    yield
    _native.set_gemm_mode(prev)


@pytest.fixture
def no_dropout():
    import vilbert.vilbert as V
    orig, V._drop_p = V._drop_p, (lambda mod: 0.0)
    yield
    V._drop_p = orig


@pytest.fixture(scope="module")
def base2():
    """bert_base_2layer_2conect, B = 4, T = 36, R = 37: config, weights, inputs, and the fp32 CPU oracle's losses and gradients
    (computed once, never modified)."""
    from oracle import vilbert_oracle as vo
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "pretraining")
    x = synth.make_inputs(cfg, B, T, R, with_labels=True)
    args = [x[n] for n in NAMES]
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k != "cls.predictions.decoder.weight"}
    leaves["cls.predictions.decoder.weight"] = leaves["bert.embeddings.word_embeddings.weight"]
    want = vo.pretraining_forward(leaves, cfg, *args)
    sum(l.sum() for l in want).backward()
    return {"cfg": cfg, "sd": sd, "args": args, "losses": [w.item() for w in want],
            "grads": {k: v.grad.double() for k, v in leaves.items() if v.grad is not None}}


def _model(case, capacity=None):
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    m = BertForMultiModalPreTraining(BertConfig.from_dict(case["cfg"]))
    m.load_state_dict(case["sd"])
    m = m.to(DEV).train()
    m.label_capacity = capacity
    return m


def _step(m, args, census=None):
    losses = m(*helpers.to_device(args, DEV))
    if census is not None:
        census.phase = "bwd"
    sum(l.sum() for l in losses).backward()
    torch.cuda.synchronize()
    return [l.item() for l in losses], {n: p.grad.detach().cpu().double() for n, p in m.named_parameters() if p.grad is not None}


class Census:
    """(launcher name, shape of the weight) of every fp32-tensor linear launch; (name, pass, element count) of every stream
    cast. The casts at the encoder's INPUT stay (the fp32 embeddings enter the stream: cast_bf16 in forward, cast_f32 of their
    gradient in backward); the casts this file is about are those of the encoder's OUTPUT: cast_f32 in forward, cast_bf16 of
    its gradient in backward. One launch of the input side has that signature too and stays: the image-feature projection
    returns fp32 [B, R, Hv] (vilbert.py BertImageEmbeddings), so its gradient is rounded by a cast_bf16 in backward."""

    def __init__(self, monkeypatch):
        from vilbert import ops, ops16
        self.linears, self.casts, self.phase = [], [], "fwd"
        real = {n: getattr(ops, n) for n in ("linear_fwd", "linear_bwd_input", "linear_bwd_weight")}
        monkeypatch.setattr(ops, "linear_fwd", lambda x, weights, *a, **k: (
            self.linears.append(("fwd", tuple(weights[0].shape))), real["linear_fwd"](x, weights, *a, **k))[1])
        monkeypatch.setattr(ops, "linear_bwd_input", lambda dy, weights, *a, **k: (
            self.linears.append(("dgrad", tuple(weights[0].shape))), real["linear_bwd_input"](dy, weights, *a, **k))[1])
        monkeypatch.setattr(ops, "linear_bwd_weight", lambda dy, x, nseg, seg_n, *a, **k: (
            self.linears.append(("wgrad", (seg_n, x.shape[-1]))), real["linear_bwd_weight"](dy, x, nseg, seg_n, *a, **k))[1])
        for name in ("cast_f32", "cast_bf16"):
            orig = getattr(ops16, name)
            monkeypatch.setattr(ops16, name, (lambda o, n: lambda x: (self.casts.append((n, self.phase, x.numel())), o(x))[1])(orig, name))

    def output_casts(self, sizes):
        return [c for c in self.casts if c[2] in sizes and (c[0], c[1]) in (("cast_f32", "fwd"), ("cast_bf16", "bwd"))]


def test_behind_the_encoder_only_the_alignment_head_is_an_fp32_tensor_linear(bf16_mode, no_dropout, base2, monkeypatch):
    cfg = base2["cfg"]
    m = _model(base2)
    census = Census(monkeypatch)
    _step(m, base2["args"], census)
    Hb, Hv = cfg["bi_hidden_size"], cfg["v_hidden_size"]
    # the 5-wide location projection of the image embedding is no head: its weight gradient has K = 5
    heads = [l for l in census.linears if l != ("wgrad", (Hv, 5))]
    assert sorted(heads) == [("dgrad", (2, Hb)), ("fwd", (2, Hb)), ("wgrad", (2, Hb))], heads
    full = {B * T * cfg["hidden_size"], B * R * Hv}
    # no cast of an encoder output or of its gradient: what is left is the gradient of the image-feature projection
    assert census.output_casts(full) == [("cast_bf16", "bwd", B * R * Hv)], census.casts
    # ... and no cast sees a whole hidden state but those at the encoder's input, one per stream and pass
    assert sorted(c for c in census.casts if c[2] in full) == sorted(
        [("cast_bf16", "fwd", n) for n in full] + [("cast_f32", "bwd", n) for n in full] + [("cast_bf16", "bwd", B * R * Hv)]), \
        census.casts


def test_the_switch_restores_the_fp32_tensor_heads_in_a_child_process(base2):
    code = """
import sys, torch
sys.path[:0] = [%r, %r]
sys.path.insert(0, %r)
import test_bf16_heads_gpu as T
from vilbert import _native, ops16
import vilbert.vilbert as V
assert not ops16.heads_enabled()
_native.set_gemm_mode("bf16")
V._drop_p = lambda mod: 0.0
class MP:
    def setattr(self, obj, name, value): setattr(obj, name, value)
""" % (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT, os.path.join(ROOT, "tests"))
    code += """
from oracle import synth
cfg = synth.load_config("bert_base_2layer_2conect.json")
case = {"cfg": cfg, "sd": synth.make_state_dict(cfg, "pretraining"),
        "args": [synth.make_inputs(cfg, T.B, T.T, T.R, with_labels=True)[n] for n in T.NAMES]}
m = T._model(case)
census = T.Census(MP())
T._step(m, case["args"], census)
shapes = sorted(set(s for kind, s in census.linears if kind == "fwd"))
print("FWD", shapes)
print("FULLCASTS", len(census.output_casts((T.B * T.T * cfg["hidden_size"], T.B * T.R * cfg["v_hidden_size"]))))
"""
    env = dict(os.environ, VB_BF16_HEADS="0")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    cfg = base2["cfg"]
    fwd = eval([l for l in out.stdout.splitlines() if l.startswith("FWD ")][0][4:])
    H, Hv, Hb = cfg["hidden_size"], cfg["v_hidden_size"], cfg["bi_hidden_size"]
    for shape in ((Hb, H), (Hb, Hv), (H, H), (Hv, Hv), (cfg["vocab_size"], H), (cfg["v_target_size"], Hv), (2, Hb)):
        assert shape in fwd, (shape, fwd)                               # poolers, transforms, decoders: the old launches
    assert int([l for l in out.stdout.splitlines() if l.startswith("FULLCASTS ")][0].split()[1]) == 5   # + 2 in forward, + 2 in backward


def _rel(got, ref, typical):
    return (got - ref).norm().item() / max(ref.norm().item(), 1e-3 * typical)


def test_oracle_parity_and_head_gradients_against_the_path_they_replace(bf16_mode, no_dropout, base2):
    """Bars of test_bf16_stream_forward_drift_and_gradient_error_are_reported. In addition, per head tensor, the relative L2
    error against the oracle may exceed that of the replaced path (VB_BF16_HEADS=0: the parent commit's computation) on the
    same inputs by at most a factor 1.5.

    The bias of the 30,522-wide decoder is the tensor this bound is tight for: its gradient is the column sum of the loss
    gradient, which at initialisation hardly depends on the logits (softmax ~ 1 / 30522 everywhere), so the replaced path - an
    fp32 sum of the fp32 gradient - is nearly exact on it (7.8e-05 measured). Summed from the bf16-rounded `G` it read 2.0e-03
    (factor 25.5); the loss backward therefore also leaves fp32 column sums of the unrounded gradient per 64 rows
    (vbh_xent_bwd_bf16 colsum_part) and the bias gradient is their ordered sum (vbh_colsum_parts)."""
    from vilbert import ops16
    m = _model(base2)
    ref = {n: base2["grads"][n] for n, _p in m.named_parameters() if n in base2["grads"]}      # (tied weights: one name)
    new_l, new_g = _step(m, base2["args"])
    prev = ops16.set_heads(False)
    try:
        old_l, old_g = _step(_model(base2), base2["args"])
    finally:
        ops16.set_heads(prev)
    for g, o, w, n in zip(new_l, old_l, base2["losses"], ("masked_lm_loss", "masked_img_loss", "next_sentence_loss")):
        print("bf16 heads, 2L/2C B=4: %s %.5f (fp32-tensor heads %.5f) vs fp32 oracle %.5f" % (n, g, o, w))
        assert abs(g - w) / abs(w) <= 2e-2, (n, g, w)
    assert set(ref) == set(new_g) == set(old_g)
    typical = sorted(g.norm().item() for g in ref.values())[len(ref) // 2]
    rel = sorted(_rel(new_g[n], g, typical) for n, g in ref.items())
    rel_old = sorted(_rel(old_g[n], g, typical) for n, g in ref.items())
    median, p90, worst = rel[len(rel) // 2], rel[len(rel) * 9 // 10], rel[-1]
    print("bf16 heads, 2L/2C B=4: gradient relative L2 vs oracle - median %.3e, p90 %.3e, worst %.3e over %d tensors "
          "(fp32-tensor heads: %.3e, %.3e, %.3e)" % (median, p90, worst, len(rel), rel_old[len(rel) // 2],
                                                     rel_old[len(rel) * 9 // 10], rel_old[-1]))
    checked, beyond = 0, []
    for n in sorted(ref):
        if n.startswith(HEAD_TENSORS):
            a, b = _rel(new_g[n], ref[n], typical), _rel(old_g[n], ref[n], typical)
            print("bf16 heads: %-48s new %.3e  fp32-tensor heads %.3e  ratio %.2f" % (n, a, b, a / b))
            if a > 1.5 * b:
                beyond.append((n, a, b))
            checked += 1
    assert checked >= 13
    assert median <= 0.05 and p90 <= 0.15 and worst <= 0.6, (median, p90, worst)
    assert median > 1e-6
    assert not beyond, beyond


def test_exact_and_fixed_capacity_gather_agree_up_to_regrouping(bf16_mode, no_dropout, base2):
    """Every row takes the same path through the same kernels under either gather; only fp32 sums over the rows (weight
    gradients, the loss means) are grouped differently: the regrouping bound of tests/test_last_layer_compact_reductions_gpu.py."""
    la, ga = _step(_model(base2, None), base2["args"])
    lb, gb = _step(_model(base2, 0.5), base2["args"])
    for a, b in zip(la, lb):
        assert abs(a - b) <= 1e-5 * abs(a), (la, lb)
    assert set(ga) == set(gb)
    gmax = max(g.abs().max().item() for g in ga.values())
    for n in ga:
        err = (ga[n] - gb[n]).abs().max().item()
        assert err <= 2e-5 * ga[n].abs().max().item() + 1e-6 * gmax, (n, err, ga[n].abs().max().item())


def test_graphed_chain_step_refreshes_the_padded_decoder_shadow_and_trains_like_eager(bf16_mode, no_dropout):
    from vilbert import ops16
    from vilbert.graphed import GraphedTrainStep
    from vilbert.optim import AdamW
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    cfg = synth.tiny_config(hidden_size=256, num_attention_heads=4, intermediate_size=512, v_feature_size=256, v_hidden_size=256,
                            v_num_attention_heads=2, v_intermediate_size=256, bi_hidden_size=256, bi_num_attention_heads=2,
                            vocab_size=211)
    sd = synth.make_state_dict(cfg, "pretraining", seed=5)
    data = [[synth.make_inputs(cfg, 8, 9, 8, seed=50 + i, with_labels=True)[n].to(DEV) for n in NAMES] for i in range(3)]

    def model():
        m = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
        m.load_state_dict(sd)
        return m.to(DEV).train()
    m0 = model()
    assert m0._bf16_heads_ok()
    o0 = AdamW(m0.parameters(), lr=2e-4, weight_decay=0.01)
    want = []
    for args in data:
        o0.zero_grad()
        loss = sum(l.mean() for l in m0(*args))
        loss.backward()
        o0.step()
        want.append(loss.item())
    m1 = model()
    o1 = AdamW(m1.parameters(), lr=2e-4, weight_decay=0.01)
    emb = m1.bert.embeddings.word_embeddings.weight
    with GraphedTrainStep(m1, o1, data[0], warmup=2, branches="chain") as step:
        got, seen = [], []
        for args in data:
            seen.append(emb.detach().clone())                           # the weights this replay's forward reads
            got.append(step(*args).item())
            step.check()
        torch.cuda.synchronize()
        entry = ops16._RAGGED._entries[(id(emb), 1)]                    # read, not fetched: a fetch would refresh it
        w16 = entry.payload["w16"]
        n = emb.shape[0]
        assert w16.shape == (ops16.padded(n), emb.shape[1]) and n == 211
        assert torch.equal(w16[:n], seen[-1].to(BF16)) and not w16[n:].any()
        assert torch.equal(entry.payload["wt16"], w16.t())
        assert not torch.equal(seen[-1], seen[0])                       # (the optimizer did move the table in between)
        assert not torch.equal(w16[:n], seen[0].to(BF16))
    print("bf16 heads, graphed (chain) vs eager losses: %s vs %s" % (got, want))
    assert got[0] == pytest.approx(want[0], rel=2e-3)
    assert got == pytest.approx(want, rel=2e-2)
