"""Deterministic mode end to end: with the ordered embedding-table backward every gradient of the model - the word table
tied to the MLM decoder, the position, token-type and task tables included - is bit-identical from run to run, and so is
every parameter after whole training steps (dropout on, AdamW), in the fp32 and the bf16 mode, for the task-token model
and for replays of the captured step. No launch may fall back to atomics on the way."""
import itertools

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "masked_lm_labels", "image_label", "image_target", "next_sentence_label"]


@pytest.fixture
def det():
    from vilbert import _native
    wanted = _native._DET["wanted"]
    _native.set_deterministic(True)
    yield _native
    _native.set_deterministic(wanted)


def _pretraining(cfg, sd):
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    m = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
    m.load_state_dict(sd)
    return m.to(DEV).train()


def _batch(cfg, batch=32, seed=7):
    x = synth.make_inputs(cfg, batch, 36, 37, seed=seed, with_labels=True)
    # two token types, so that both rows of the type table take contended sums
    x["token_type_ids"] = (torch.arange(36)[None, :] >= 18).long().expand(batch, 36).contiguous()
    return [x[n].to(DEV) for n in NAMES]


def _restart_dropout_seeds():
    import vilbert.autograd_ops as AO
    torch.manual_seed(20261016)
    AO._seed_counter = itertools.count(1)


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for n in a:
        assert torch.equal(a[n], b[n]), "%s: %s differs between the two runs" % (what, n)


def test_every_gradient_is_bit_identical_across_two_backward_passes(det):
    import vilbert.vilbert as V
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "pretraining")
    args = _batch(cfg)
    orig, V._drop_p = V._drop_p, (lambda m: 0.0)
    try:
        m = _pretraining(cfg, sd)
        grads = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            before = det.deterministic_fallbacks()
            sum(l.mean() for l in m(*args)).backward()
            torch.cuda.synchronize()
            assert det.deterministic_fallbacks() == before
            grads.append({n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None})
    finally:
        V._drop_p = orig
    assert any("word_embeddings" in n for n in grads[0]) and any("token_type_embeddings" in n for n in grads[0])
    assert len(grads[0]) > 150
    _assert_same(grads[0], grads[1], "gradient")


def _train(model, args_list, bf16=False):
    from vilbert.optim import AdamW
    if bf16:
        model.half()
    opt = AdamW(model.parameters(), lr=1e-3, weight_decay=0.01)
    _restart_dropout_seeds()
    for args in args_list:
        opt.zero_grad(set_to_none=True)
        loss = sum(l.mean() for l in model(*args))
        loss.backward()
        opt.step()
    torch.cuda.synchronize()
    return {n: p.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_training_steps_with_dropout_are_bit_identical(det, bf16):
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "pretraining")
    data = [_batch(cfg, seed=11 + i) for i in range(2)]
    before = det.deterministic_fallbacks()
    a = _train(_pretraining(cfg, sd), data, bf16)
    b = _train(_pretraining(cfg, sd), data, bf16)
    assert det.deterministic_fallbacks() == before
    assert not torch.equal(a["bert.embeddings.word_embeddings.weight"], sd["bert.embeddings.word_embeddings.weight"].to(DEV))
    _assert_same(a, b, "parameter")


def test_task_token_model_step_is_bit_identical(det):
    from vilbert.optim import AdamW
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    cfg = dict(synth.load_config("bert_base_2layer_2conect.json"), task_specific_tokens=True)
    sd = synth.make_state_dict(cfg, "vltasks")
    x = synth.make_inputs(cfg, 16, 36, 37, seed=9, task_id=3)
    x["task_ids"][::2] = 5
    args = [x[n].to(DEV) for n in ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask",
                                   "image_attention_mask", "co_attention_mask", "task_ids")]

    def run():
        m = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
        m.load_state_dict(sd)
        m = m.to(DEV).train()
        opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
        _restart_dropout_seeds()
        for _ in range(2):
            opt.zero_grad(set_to_none=True)
            out = m(*args)[:9]
            sum(o.float().mean() for i, o in enumerate(out) if i != 6).backward()
            opt.step()
        torch.cuda.synchronize()
        assert m.bert.embeddings.task_embeddings.weight.grad is not None
        return {n: p.detach().clone() for n, p in m.named_parameters()}

    before = det.deterministic_fallbacks()
    a, b = run(), run()
    assert det.deterministic_fallbacks() == before
    assert not torch.equal(a["bert.embeddings.task_embeddings.weight"],
                           sd["bert.embeddings.task_embeddings.weight"].to(DEV))
    _assert_same(a, b, "parameter")


def test_graphed_step_replays_are_bit_identical(det):
    from vilbert.graphed import GraphedTrainStep
    from vilbert.optim import AdamW
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    sd = synth.make_state_dict(cfg, "pretraining")
    data = [_batch(cfg, batch=8, seed=21 + i) for i in range(2)]

    def run():
        m = _pretraining(cfg, sd)
        opt = AdamW(m.parameters(), lr=1e-3, weight_decay=0.01)
        _restart_dropout_seeds()
        with GraphedTrainStep(m, opt, data[0], warmup=2) as step:
            losses = [step(*args).item() for args in data]
            step.check()
        torch.cuda.synchronize()
        return losses, {n: p.detach().clone() for n, p in m.named_parameters()}

    before = det.deterministic_fallbacks()
    (la, a), (lb, b) = run(), run()
    assert det.deterministic_fallbacks() == before
    assert la == lb
    _assert_same(a, b, "parameter")
