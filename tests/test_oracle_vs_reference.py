"""Pins oracle/ (restatement + parameter table) against the REAL reference model: the state_dict table, the tiny
model's forward outputs and the pre-training losses and gradients.

Everywhere: against values recorded from the reference (tests/golden/reference_pins.{json,npz}, written by
tests/golden/make_reference_pins.py - float arrays as strided samples with the whole array's shape and largest
|value|, so the tolerances are the same). Where the reference tree is present: also against every element the
reference itself computes."""
import pytest
import torch

from helpers import cases
from oracle import ref_loader, synth, vilbert_oracle as vo

import make_reference_pins as mrp


@pytest.fixture(scope="module")
def pins():
    return cases.load_pins()


@pytest.mark.parametrize("kind", ["pretraining", "vltasks"])
@pytest.mark.parametrize("cfgname", ["tiny", "tiny_task", "bert_base_2layer_2conect.json"])
def test_param_table_matches_reference_state_dict(kind, cfgname, pins):
    want = [(k, tuple(s)) for k, s in pins[0]["state_dict"]["%s/%s" % (kind, cfgname)]]
    got = [(n, tuple(s)) for n, s, _ in synth.param_table(mrp.state_dict_cfg(cfgname), kind)]
    assert got == want


def _close(a, b, tol):
    assert a.shape == b.shape
    err = (a - b).abs().max().item()
    assert err <= tol, err


def _pinned_close(a, pin, tol):
    err = cases.pin_error(a, pin)
    assert err <= tol, err


def _forward_matches(tag, case, arrays):
    cfg, sd, args = case
    with torch.no_grad():
        got = vo.vltasks_forward(sd, cfg, *args)
    for i, g in enumerate(got[:9]):
        pin = arrays["%s/%d" % (tag, i)]
        _pinned_close(g, pin, 2e-6 * max(1.0, pin.absmax))
    if ref_loader.available():
        for g, w in zip(got, mrp.reference_vltasks(cfg, sd, args)):
            _close(g, w, 2e-6 * max(1.0, w.abs().max().item()))


def test_vltasks_forward_matches_reference(pins):
    _forward_matches("vltasks_forward", mrp.vltasks_case(), pins[1])


def test_task_tokens_and_odd_batch(pins):
    _forward_matches("task_tokens", mrp.task_tokens_case(), pins[1])


@pytest.mark.parametrize("visual_target", [0, 1])
def test_pretraining_losses_and_grads_match_reference(visual_target, pins):
    cfg, sd, args = mrp.pretraining_case(visual_target)
    arrays = pins[1]
    leaves = {k: v.clone().requires_grad_(True) for k, v in sd.items() if not k.endswith("decoder.weight") or "image" in k}
    leaves["cls.predictions.decoder.weight"] = leaves["bert.embeddings.word_embeddings.weight"]
    got = vo.pretraining_forward(leaves, cfg, *args)
    sum(l.sum() for l in got).backward()
    for i, g in enumerate(got):
        _pinned_close(g.detach(), arrays["pretraining_vt%d/loss/%d" % (visual_target, i)], 1e-5)
    prefix = "pretraining_vt%d/grad/" % visual_target
    no_grad = pins[0]["pretraining_vt%d_no_grad" % visual_target]
    for name in no_grad:
        assert leaves[name].grad is None or leaves[name].grad.abs().max() == 0, name
    n = 0
    for key, pin in arrays.items():
        if key.startswith(prefix):
            _pinned_close(leaves[key[len(prefix):]].grad, pin, 1e-5 * max(1.0, pin.absmax))
            n += 1
    assert n > 0
    if ref_loader.available():
        want_losses, want_grads = mrp.reference_pretraining(cfg, sd, args)
        for g, w in zip(got, want_losses):
            _close(g.detach(), w, 1e-5)
        for name, w in want_grads.items():
            if w is None:
                assert leaves[name].grad is None or leaves[name].grad.abs().max() == 0, name
            else:
                _close(leaves[name].grad, w, 1e-5 * max(1.0, w.abs().max().item()))
