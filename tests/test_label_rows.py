"""The label-row builder and the region-loss tail all three pre-training loss routes share
(vilbert.BertForMultiModalPreTraining: _label_rows, _region_loss), in plain torch on the CPU, on the labels of
tests/test_last_layer_rows.py. Visual targets 0 and 2 need the device: tests/test_nce_loss_gpu.py and
tests/test_bf16_heads_gpu.py compare their routes there."""
import pytest
import torch

from oracle import synth
from test_last_layer_rows import B, R, _labels, _model

FIELDS = ("idx_t", "labels_t", "idx_r", "valid_r", "divisor_r", "n_t", "n_r")


@pytest.fixture(autouse=True)
def no_capture(monkeypatch):
    """_static_gather() asks the HIP runtime whether a graph capture is in progress: none is, and there may be no device."""
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)


def test_exact_gather_returns_the_nonzero_rows():
    lm, il = _labels()
    m = _model()
    assert m.label_capacity is None
    rows = m._label_rows(lm, il)
    assert rows._fields == FIELDS
    assert torch.equal(rows.idx_t, torch.nonzero(lm.reshape(-1) != -1).squeeze(1))
    assert torch.equal(rows.idx_r, torch.nonzero(il.reshape(-1) == 1).squeeze(1))
    assert torch.equal(rows.labels_t, lm.reshape(-1)[rows.idx_t])
    assert rows.valid_r is None
    assert type(rows.divisor_r) is float and rows.divisor_r == 4.0
    assert (type(rows.n_t), rows.n_t, type(rows.n_r), rows.n_r) == (int, 5, int, 4)
    assert m._label_rows(torch.full_like(lm, -1), il) is None           # no token labelled
    assert m._label_rows(lm, torch.zeros_like(il)) is None              # no region labelled


def test_static_gather_returns_the_record_of_static_label_rows():
    lm, il = _labels()
    m = _model()
    m.label_capacity = 0.5
    got, want = m._label_rows(lm, il), m._static_label_rows(lm, il)
    assert got._fields == FIELDS and type(got) is type(want)
    for name in FIELDS:
        assert torch.equal(getattr(got, name), getattr(want, name)), name
    assert got.valid_r.numel() > 4 and got.valid_r.sum() == 4          # padded


def test_auto_measures_the_capacity_on_the_first_call():
    lm, il = _labels()
    m = _model()
    m.label_capacity = "auto"
    first = m._label_rows(lm, il)
    assert first.valid_r is None and type(first.divisor_r) is float     # the exact gather
    frac = max(int((lm != -1).sum()) / lm.numel(), int((il == 1).sum()) / il.numel())
    assert m._auto_capacity == min(1.0, 1.2 * frac + 0.01)
    second = m._label_rows(lm, il)
    assert second.valid_r is not None and torch.is_tensor(second.divisor_r) and torch.is_tensor(second.n_r)
    assert m._auto_capacity == min(1.0, 1.2 * frac + 0.01)


def test_region_loss_of_target_1_ignores_the_padding_rows():
    """Squared error on a padded fixed-capacity record against the exact record on the same scores. rtol 1e-6: both are one
    fp32 sum of at most 4 * R * dim terms, grouped differently (the padding rows add exact zeros)."""
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    dim = 8
    lm, il = _labels()
    m = BertForMultiModalPreTraining(BertConfig.from_dict(synth.tiny_config(visual_target=1, v_target_size=dim)))
    exact = m._label_rows(lm, il)
    m.label_capacity = 0.5
    static = m._label_rows(lm, il)
    n, cap = exact.idx_r.numel(), static.idx_r.numel()
    assert cap > n
    g = torch.Generator().manual_seed(2)
    image_target = torch.randn(B, R, dim, generator=g)
    scores = torch.randn(cap, dim, generator=g)
    assert (scores[n:] != 0).all()                                      # arbitrary nonzero scores on the padding rows
    scores.requires_grad_(True)
    want = m._region_loss(scores[:n], image_target, exact, il)
    got = m._region_loss(scores, image_target, static, il)
    torch.testing.assert_close(got, want, rtol=1e-6, atol=0.0)
    # the reference's expression on the whole [B, R, dim] block (reference vilbert.py:1506-1512)
    full = torch.zeros(B * R, dim).index_copy(0, exact.idx_r, scores[:n].detach()).reshape(B, R, dim)
    mask = (il == 1).unsqueeze(2).float()
    ref = torch.sum((full - image_target) ** 2 * mask) / max(torch.sum(mask.expand(-1, -1, dim)), 1)
    torch.testing.assert_close(want, ref, rtol=1e-6, atol=0.0)
    got.backward()
    assert scores.grad[:n].abs().min() > 0 and torch.equal(scores.grad[n:], torch.zeros(cap - n, dim))
