"""bf16 training mode, fine-tuning wrapper: the heads of VILBertForVLTasks on the bf16 stream and the head selection
(`set_active_heads`); csrc/finetune16.hip, tests/test_finetune16_gpu.py holds its kernels.

  * launch census: on a bf16 training step no cast sees a whole encoder output (or its gradient) and neither the two 1-wide
    logits nor the two decoders are fp32-tensor linears; ops16.set_heads(False) brings those launches and casts back;
  * parity with the fp32 CPU oracle, per output and per parameter gradient, against the path this one replaces
    (ops16.set_heads(False), same inputs): at most 1.5 x its relative L2 error;
  * selection: for every task type of the reference's trainer the one head it reads is bit-equal to the all-heads forward's
    and everything else is None - fp32 eval, fp32 train, bf16 train -, no decoder is launched unless a `*_prediction` of
    `cls` is selected, and the odd-batch leak of the alignment score survives;
  * dropout: the masks of a selected head do not depend on the selection, a step repeats bit for bit from the same seeds,
    and a captured step replays the eager loss."""
import itertools
import math

import pytest
import torch

import helpers
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
NAMES = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "co_attention_mask")
HEADS = ("vil_prediction", "vil_prediction_gqa", "vil_logit", "vil_binary_prediction", "vil_tri_prediction",
         "vision_prediction", "vision_logit", "linguisic_prediction", "linguisic_logit")
TASK_TYPES = ("VL-classifier", "VL-classifier-GQA", "VL-logit", "V-logit", "V-logit-mc", "VL-binary-classifier",
              "VL-tri-classifier")
B, T, R = 4, 12, 11
# the parameters whose gradient the route computes differently
ROUTE_TENSORS = ("bert.t_pooler.dense.", "bert.v_pooler.dense.", "cls.predictions.transform.", "cls.imagePredictions.transform.",
                 "cls.predictions.bias", "cls.imagePredictions.decoder.", "bert.embeddings.word_embeddings.weight",
                 "vision_logit.", "linguisic_logit.")


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


def _loss_weights(outputs, seed=77):
    """One fixed random fp32 tensor per output: the loss sum_i (out_i * w_i).sum() gives every head a gradient."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(o.shape, generator=g) for o in outputs]


def _loss(outputs, weights):
    return sum((o * w.to(o.device)).sum() for o, w in zip(outputs, weights) if o is not None)


@pytest.fixture(scope="module")
def base2():
    """bert_base_2layer_2conect, B = 4, T = 12, R = 11, ragged masks: config, weights, inputs, the loss weights, and the fp32
    CPU oracle's nine outputs and parameter gradients (computed once, never modified)."""
    from oracle import vilbert_oracle as vo
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "vltasks")
    x = synth.make_inputs(cfg, B, T, R)
    args = [x[n] for n in NAMES]
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if k != "cls.predictions.decoder.weight"}
    leaves["cls.predictions.decoder.weight"] = leaves["bert.embeddings.word_embeddings.weight"]
    want = vo.vltasks_forward(leaves, cfg, *args)
    weights = _loss_weights(want)
    _loss(want, weights).backward()
    return {"cfg": cfg, "sd": sd, "args": args, "weights": weights, "outputs": [w.detach().double() for w in want],
            "grads": {k: v.grad.double() for k, v in leaves.items() if v.grad is not None}}


def _model(cfg, sd, train=True):
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    m = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
    m.load_state_dict(sd)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _step(m, args, weights, census=None):
    out = m(*helpers.to_device(args, DEV))[:9]
    if census is not None:
        census.phase = "bwd"
    _loss(out, weights).backward()
    torch.cuda.synchronize()
    return ([o.detach().cpu().double() for o in out],
            {n: p.grad.detach().cpu().double() for n, p in m.named_parameters() if p.grad is not None})


class Census:
    """The method of tests/test_bf16_heads_gpu.py: (pass, shape of the weight, rows) of every fp32-tensor linear launch and (name,
    pass, element count) of every stream cast; in addition (launcher, shape of the weight) of every bf16 linear forward, the ragged
    one included - `decoders()` finds a decoder launch of any kind."""

    def __init__(self, monkeypatch):
        from vilbert import ops, ops16
        self.linears, self.casts, self.linears16, self.phase = [], [], [], "fwd"
        real = {n: getattr(ops, n) for n in ("linear_fwd", "linear_bwd_input", "linear_bwd_weight")}
        monkeypatch.setattr(ops, "linear_fwd", lambda x, weights, *a, **k: (
            self.linears.append(("fwd", tuple(weights[0].shape), x.numel() // x.shape[-1])), real["linear_fwd"](x, weights, *a, **k))[1])
        monkeypatch.setattr(ops, "linear_bwd_input", lambda dy, weights, *a, **k: (
            self.linears.append(("dgrad", tuple(weights[0].shape), dy.numel() // dy.shape[-1])),
            real["linear_bwd_input"](dy, weights, *a, **k))[1])
        monkeypatch.setattr(ops, "linear_bwd_weight", lambda dy, x, nseg, seg_n, *a, **k: (
            self.linears.append(("wgrad", (seg_n, x.shape[-1]), x.numel() // x.shape[-1])),
            real["linear_bwd_weight"](dy, x, nseg, seg_n, *a, **k))[1])
        for name in ("cast_f32", "cast_bf16"):
            orig = getattr(ops16, name)
            monkeypatch.setattr(ops16, name, (lambda o, n: lambda x: (self.casts.append((n, self.phase, x.numel())), o(x))[1])(orig, name))
        fwd16, ragged = ops16.linear_fwd, ops16.linear_ragged_fwd
        monkeypatch.setattr(ops16, "linear_fwd", lambda x, weights, *a, **k: (
            self.linears16.append(("fwd16", tuple(weights[0].shape))), fwd16(x, weights, *a, **k))[1])
        monkeypatch.setattr(ops16, "linear_ragged_fwd", lambda x, weight, *a, **k: (
            self.linears16.append(("ragged", tuple(weight.shape))), ragged(x, weight, *a, **k))[1])

    def clear(self):
        del self.linears[:], self.casts[:], self.linears16[:]
        self.phase = "fwd"

    def output_casts(self, sizes):
        return [c for c in self.casts if c[2] in sizes and (c[0], c[1]) in (("cast_f32", "fwd"), ("cast_bf16", "bwd"))]

    def decoders(self, cfg):
        shapes = ((cfg["vocab_size"], cfg["hidden_size"]), (cfg["v_target_size"], cfg["v_hidden_size"]))
        return [l for l in self.linears + self.linears16 if l[1] in shapes]


def test_no_cast_of_an_encoder_output_and_no_fp32_tensor_linear_for_logits_and_decoders(bf16_mode, no_dropout, base2, monkeypatch):
    from vilbert import ops16
    cfg = base2["cfg"]
    H, Hv = cfg["hidden_size"], cfg["v_hidden_size"]
    full = {B * T * H, B * R * Hv}
    # (in this config bi_hidden_size == v_hidden_size: `vil_logit`, a pooled head over B rows that stays an fp32-tensor linear,
    # has the weight shape of `vision_logit` - the launches in question are those over all token / region rows)
    gone = {((1, H), B * T), ((1, Hv), B * R), ((cfg["vocab_size"], H), B * T), ((cfg["v_target_size"], Hv), B * R)}
    m = _model(cfg, base2["sd"])
    assert m._bf16_heads_ok()
    census = Census(monkeypatch)
    _step(m, base2["args"], base2["weights"], census)
    # no cast of an encoder output or of its gradient: what is left is the gradient of the image-feature projection (the
    # encoder-input cast tests/test_bf16_heads_gpu.py documents) ...
    assert census.output_casts(full) == [("cast_bf16", "bwd", B * R * Hv)], census.casts
    # ... and no cast sees a whole hidden state but those at the encoder's input, one per stream and pass
    assert sorted(c for c in census.casts if c[2] in full) == sorted(
        [("cast_bf16", "fwd", n) for n in full] + [("cast_f32", "bwd", n) for n in full] + [("cast_bf16", "bwd", B * R * Hv)]), \
        census.casts
    assert not [l for l in census.linears if l[1:] in gone], census.linears
    # the decoders did run, on the bf16 kernels
    assert sorted(l[:2] for l in census.decoders(cfg)) == [("ragged", (cfg["v_target_size"], Hv)), ("ragged", (cfg["vocab_size"], H))]

    # the switch restores the fp32-tensor heads: those launches (forward, input gradient, weight gradient) and casts are back
    prev = ops16.set_heads(False)
    try:
        census.clear()
        _step(_model(cfg, base2["sd"]), base2["args"], base2["weights"], census)
    finally:
        ops16.set_heads(prev)
    for shape, rows in gone:
        for kind in ("fwd", "dgrad", "wgrad"):
            assert (kind, shape, rows) in census.linears, (kind, shape, rows, census.linears)
    assert len(census.output_casts(full)) == 5, census.casts      # + 2 in forward, + 2 in backward
    assert not [l for l in census.linears16 if l[0] == "ragged"]


def _rel(got, ref, typical):
    return (got - ref).norm().item() / max(ref.norm().item(), 1e-3 * typical)


def _ratio(a, b):
    """For the printed table only: a / b, 1 for 0 / 0."""
    return a / b if b > 0 else (1.0 if a == 0 else float("inf"))


def test_oracle_parity_of_outputs_and_head_gradients_against_the_path_they_replace(bf16_mode, no_dropout, base2):
    """Per output and per head tensor, the relative L2 error against the fp32 CPU oracle may exceed that of the replaced path
    (ops16.set_heads(False): the parent commit's computation) on the same inputs by at most the factor 1.5 of
    tests/test_bf16_heads_gpu.py, with its `_rel` and `typical` (0 against 0 - a gradient bit-equal to the oracle's on both
    paths - passes). The table this prints is in DESIGN.md section 7."""
    from vilbert import ops16
    cfg = base2["cfg"]
    m = _model(cfg, base2["sd"])
    ref = {n: base2["grads"][n] for n, _p in m.named_parameters() if n in base2["grads"]}      # (tied weights: one name)
    new_o, new_g = _step(m, base2["args"], base2["weights"])
    prev = ops16.set_heads(False)
    try:
        old_o, old_g = _step(_model(cfg, base2["sd"]), base2["args"], base2["weights"])
    finally:
        ops16.set_heads(prev)
    assert set(ref) == set(new_g) == set(old_g)
    beyond, checked = [], 0
    typical_o = sorted(o.norm().item() for o in base2["outputs"])[len(HEADS) // 2]
    for name, g, o, w in zip(HEADS, new_o, old_o, base2["outputs"]):
        assert g.shape == w.shape and torch.isfinite(g).all(), name
        a, b = _rel(g, w, typical_o), _rel(o, w, typical_o)
        print("bf16 fine-tuning heads: output %-40s new %.3e  fp32-tensor heads %.3e  ratio %.2f" % (name, a, b, _ratio(a, b)))
        if a > 1.5 * b:
            beyond.append((name, a, b))
    typical = sorted(g.norm().item() for g in ref.values())[len(ref) // 2]
    rel = sorted(_rel(new_g[n], g, typical) for n, g in ref.items())
    rel_old = sorted(_rel(old_g[n], g, typical) for n, g in ref.items())
    print("bf16 fine-tuning heads, 2L/2C B=4: gradient relative L2 vs oracle - median %.3e, p90 %.3e, worst %.3e over %d tensors "
          "(fp32-tensor heads: %.3e, %.3e, %.3e)" % (rel[len(rel) // 2], rel[len(rel) * 9 // 10], rel[-1], len(rel),
                                                     rel_old[len(rel) // 2], rel_old[len(rel) * 9 // 10], rel_old[-1]))
    for n in sorted(ref):
        if n.startswith(ROUTE_TENSORS):
            a, b = _rel(new_g[n], ref[n], typical), _rel(old_g[n], ref[n], typical)
            print("bf16 fine-tuning heads: %-48s new %.3e  fp32-tensor heads %.3e  ratio %.2f" % (n, a, b, _ratio(a, b)))
            if a > 1.5 * b:
                beyond.append((n, a, b))
            checked += 1
    assert checked >= 17
    assert rel[len(rel) // 2] > 1e-6
    assert not beyond, beyond


def _select_and_compare(m, args, census=None, cfg=None):
    """All heads once, then each task type's head alone: None everywhere else, the selected output bit-equal."""
    from vilbert.task_losses import HEAD_OF_TASK_TYPE
    m.set_active_heads(None)
    everything = m(*args)
    assert all(o is not None for o in everything[:9])
    for task_type in TASK_TYPES:
        name = HEAD_OF_TASK_TYPE[task_type]
        m.set_active_heads([name])
        if census is not None:
            census.clear()
        got = m(*args)
        assert len(got) == 10
        for i, head in enumerate(HEADS):
            if head == name:
                assert got[i] is not None and got[i].shape == everything[i].shape
                assert torch.equal(got[i], everything[i]), (task_type, head)
            else:
                assert got[i] is None, (task_type, head)
        if census is not None:
            assert not census.decoders(cfg), (task_type, census.decoders(cfg))
    if census is not None:      # a `*_prediction` of cls is selected: its decoder runs, and only it
        for name, shape in (("linguisic_prediction", (cfg["vocab_size"], cfg["hidden_size"])),
                            ("vision_prediction", (cfg["v_target_size"], cfg["v_hidden_size"]))):
            m.set_active_heads([name])
            census.clear()
            got = m(*args)
            assert torch.equal(got[HEADS.index(name)], everything[HEADS.index(name)])
            assert [l[1] for l in census.decoders(cfg)] == [shape], census.decoders(cfg)
    m.set_active_heads(None)


def test_selection_fp32_eval_and_train(no_dropout, base2, monkeypatch):
    args = helpers.to_device(base2["args"], DEV)
    census = Census(monkeypatch)
    m = _model(base2["cfg"], base2["sd"], train=False)
    with torch.no_grad():
        _select_and_compare(m, args, census, base2["cfg"])
    _select_and_compare(m.train(), args, census, base2["cfg"])


def test_selection_bf16_train(bf16_mode, no_dropout, base2, monkeypatch):
    args = helpers.to_device(base2["args"], DEV)
    census = Census(monkeypatch)
    _select_and_compare(_model(base2["cfg"], base2["sd"]), args, census, base2["cfg"])
    assert not census.output_casts({B * T * base2["cfg"]["hidden_size"], B * R * base2["cfg"]["v_hidden_size"]})


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_odd_batch_leaks_the_alignment_score_under_selection_too(mode, no_dropout, base2):
    from vilbert import _native
    cfg = base2["cfg"]
    x = synth.make_inputs(cfg, 3, T, R)
    args = helpers.to_device([x[n] for n in NAMES], DEV)
    prev = _native.set_gemm_mode(mode)
    try:
        m = _model(cfg, base2["sd"])
        everything = m(*args)
        assert everything[3].shape == (3, 2)                   # the 2-wide alignment score, not the pair classifier's output
        m.set_active_heads(["vil_binary_prediction"])
        got = m(*args)
        assert torch.equal(got[3], everything[3]) and all(got[i] is None for i in range(9) if i != 3)
    finally:
        _native.set_gemm_mode(prev)


# ---- dropout on: a small configuration the route takes (the hidden_size = 256 one of tests/test_bf16_heads_gpu.py) ---------------
def _small():
    cfg = synth.tiny_config(hidden_size=256, num_attention_heads=4, intermediate_size=512, v_feature_size=256, v_hidden_size=256,
                            v_num_attention_heads=2, v_intermediate_size=256, bi_hidden_size=256, bi_num_attention_heads=2,
                            vocab_size=211)
    sd = synth.make_state_dict(cfg, "vltasks", seed=5)
    args = [synth.make_inputs(cfg, 8, 9, 8, seed=50)[n].to(DEV) for n in NAMES]
    return cfg, sd, args


def _peek_seed_counter():
    from vilbert import autograd_ops as A
    v = next(A._seed_counter)
    A._seed_counter = itertools.count(v)
    return v


def _set_seed_counter(v):
    from vilbert import autograd_ops as A
    A._seed_counter = itertools.count(v)


@pytest.mark.parametrize("mode", ["f32", "bf16"])
def test_dropout_masks_of_a_selected_head_do_not_depend_on_the_selection(mode):
    from vilbert import _native
    cfg, sd, args = _small()
    prev = _native.set_gemm_mode(mode)
    try:
        m = _model(cfg, sd)
        assert mode == "f32" or m._bf16_heads_ok()
        _set_seed_counter(5000)
        everything = m(*args)
        _set_seed_counter(5000)
        again = m(*args)
        _set_seed_counter(6000)
        other = m(*args)
        for name in ("vil_logit", "vision_logit", "linguisic_logit", "vil_binary_prediction"):
            i = HEADS.index(name)
            assert torch.equal(everything[i], again[i]) and not torch.equal(everything[i], other[i]), name     # dropout is on
            m.set_active_heads([name])
            _set_seed_counter(5000)
            got = m(*args)
            assert torch.equal(got[i], everything[i]), name
            assert all(got[j] is None for j in range(9) if j != i)
        m.set_active_heads(None)
    finally:
        _native.set_gemm_mode(prev)


def test_two_runs_from_the_same_seeds_are_bit_identical(bf16_mode):
    cfg, sd, args = _small()
    m = _model(cfg, sd)
    assert m._bf16_heads_ok()
    with torch.no_grad():
        weights = _loss_weights(m(*args)[:9])
    runs = []
    for start in (7000, 7000, 8000):
        _set_seed_counter(start)
        m.zero_grad(set_to_none=True)
        loss = _loss(m(*args)[:9], weights)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((loss.item(), {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}))
    (la, ga), (lb, gb), (lc, _gc) = runs
    assert la == lb and la != lc
    assert set(ga) == set(gb) and "vision_logit.weight" in ga and "linguisic_logit.bias" in ga
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n


def test_graphed_step_over_the_route_replays_the_eager_loss():
    """Dropout on, frozen weights (lr = 0): replay r of the captured step draws the masks of (the host seeds of the capture, device
    step counter r). An eager step from the same host seeds under a registered counter holding r computes the same loss."""
    from vilbert import _native as N
    from vilbert.graphed import GraphedTrainStep
    from vilbert.optim import AdamW
    cfg, sd, args = _small()
    prev = N.set_gemm_mode("bf16")
    try:
        m = _model(cfg, sd)
        assert m._bf16_heads_ok()
        with torch.no_grad():
            weights = [w.to(DEV) for w in _loss_weights(m(*args)[:9])]
        loss_fn = lambda out: _loss(out[:9], weights)
        opt = AdamW(m.parameters(), lr=0.0)
        n0 = _peek_seed_counter()
        with GraphedTrainStep(m, opt, args, loss_fn=loss_fn, warmup=2, branches="chain") as step:
            n1 = _peek_seed_counter()
            per_step, rest = divmod(n1 - n0, 3)          # two warm-up steps and the capture draw the same number of seeds
            assert rest == 0 and per_step >= 4
            got = [step(*args).item() for _ in range(2)]
            torch.cuda.synchronize()
        assert all(math.isfinite(l) for l in got) and got[0] != got[1]      # fresh masks every replay
        want = []
        for epoch in (1, 2):
            counter = torch.tensor([epoch], dtype=torch.int64, device=DEV)
            N.check(N.lib().vb_set_seed_epoch(counter.data_ptr()), "vb_set_seed_epoch")
            try:
                _set_seed_counter(n1 - per_step)
                m.zero_grad(set_to_none=True)
                loss = loss_fn(m(*args))
                loss.backward()
                want.append(loss.item())
                torch.cuda.synchronize()
            finally:
                N.lib().vb_set_seed_epoch(None)
        print("bf16 fine-tuning heads, graphed (chain) vs eager losses: %s vs %s" % (got, want))
        assert got == pytest.approx(want, rel=1e-6)        # the same deterministic kernels from the same seeds
    finally:
        N.set_gemm_mode(prev)
