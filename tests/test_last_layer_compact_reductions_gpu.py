"""Backward of an output + feed-forward block on a row map (csrc/layers.hip ffn_block_rows_bwd): the LayerNorm backwards, their
column reduces and the three weight / bias gradients run on the COMPACT rows, so their sums over rows are grouped differently
from the whole block's - every other term is an exact zero there and absent here. Against the same layer without a map
(layers.self_layer, as tests/test_last_layer_rows_gpu.py): dx of every row and all 16 parameter gradients.

Bounds: tests/test_last_layer_rows_gpu.py::_close, 2e-5 x max|want| + 1e-6 x global max (the project's bound for a reordering
of fp32 sums of this size).

A padding entry of the map has a zero dy row and must add exact zeros to every reduction; 0 * x is zero only for a finite
x, so the mapped runs start from temporaries filled with NaN bit patterns: a forward buffer of a padding row that no kernel
writes (sum1, sum2, a1, h, ctx_rows, the statistics) would show as a NaN gradient."""
import itertools

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, want, gmax, what):
    err = (got - want).abs().max().item()
    if err > 0.0:
        print("%s: max diff %.3e (max %.3e)" % (what, err, want.abs().max().item()))
    assert err <= 2e-5 * want.abs().max().item() + 1e-6 * gmax, "%s: max diff %.3e" % (what, err)


class _Block(object):
    """One BertLayer, dropout 0.1 on all three dropouts, parameters away from their defaults; run(rows) = one forward +
    backward with the seed counter restarted, so every run draws the same masks."""

    def __init__(self, B, S, H, I, seed):
        from vilbert.vilbert import BertConfig, BertLayer
        cfg = synth.tiny_config(hidden_size=H, num_attention_heads=1, intermediate_size=I)
        torch.manual_seed(seed)
        self.layer = BertLayer(BertConfig.from_dict(cfg)).to(DEV).train()
        for p in self.layer.parameters():
            p.data.add_(torch.randn_like(p) * 0.05)
        self.B, self.S, self.H = B, S, H
        self.x0 = torch.randn(B, S, H, device=DEV)
        self.mask = torch.zeros(B, 1, 1, S, device=DEV)
        self.mask[1, 0, 0, S - 1] = -10000.0
        self.w_full = torch.randn(B * S, H, device=DEV)      # the readers' weights, by row of the full tensor

    def run(self, rows, mapped, poison=False):
        """rows: int32 map; mapped: through the map, or the whole layer read at the rows the map names."""
        import vilbert.autograd_ops as AO
        from vilbert import layers
        valid = rows >= 0
        src = rows.to(torch.int64).clamp(min=0)
        w = self.w_full.index_select(0, src) * valid.unsqueeze(1)             # (a padding entry never gets a gradient)
        AO._seed_counter = itertools.count(1)
        x = self.x0.clone().requires_grad_(True)
        for p in self.layer.parameters():
            p.grad = None
        alloc0 = layers._Carver.alloc
        if poison:
            layers._Carver.alloc = lambda c, device: alloc0(c, device).fill_(0xFF)
        try:
            y = layers.self_layer(self.layer, x, self.mask, 0.1, 0.1, 0.1, rows if mapped else None)
            assert y is not None
            picked = y if mapped else y.reshape(-1, self.H).index_select(0, src)
            (picked * w).sum().backward()
            torch.cuda.synchronize()
        finally:
            layers._Carver.alloc = alloc0
        return x.grad.clone(), {n: p.grad.clone() for n, p in self.layer.named_parameters()}

    def compare(self, rows):
        dx_all, g_all = self.run(rows, mapped=False)
        dx_map, g_map = self.run(rows, mapped=True, poison=True)
        assert set(g_map) == set(g_all) and len(g_all) == 16
        assert torch.isfinite(dx_map).all()
        for n, g in g_map.items():
            assert torch.isfinite(g).all(), n
        gmax = max(g.abs().max().item() for g in g_all.values())
        _close(dx_map, dx_all, gmax, "dx")
        for n, g in g_all.items():
            assert g.abs().max().item() > 0.0, n
            _close(g_map[n], g, gmax, n)


@pytest.fixture(scope="module")
def block():
    return _Block(5, 37, 64, 96, seed=11)


def _map64(named):
    """64 entries: the named rows in order, padding in between (after every fourth named entry, so padding lies between named
    entries wherever there are more than four) and behind."""
    out = []
    for i, r in enumerate(named):
        out.append(r)
        if i % 4 == 3:
            out.append(-1)
    assert len(out) <= 64
    return torch.tensor(out + [-1] * (64 - len(out)), dtype=torch.int32, device=DEV)


def test_contraction_across_several_k_tiles_with_padding_between_named_entries(block):
    """64 compact rows = four 16-row K tiles of the weight gradients: the 5 pooler rows, 20 more rows in no order, 39 padding
    entries, 6 of them between named entries."""
    pool = [b * block.S for b in range(block.B)]
    more = [151, 3, 36, 38, 73, 75, 110, 112, 184, 20, 99, 64, 1, 147, 149, 50, 128, 17, 90, 183]
    rows = _map64(pool + more)
    named = rows[rows >= 0].tolist()
    assert len(named) == 25 and len(set(named)) == 25 and int((rows < 0).sum()) == 39
    last = max(i for i, r in enumerate(rows.tolist()) if r >= 0)
    assert int((rows[:last] < 0).sum()) >= 3
    block.compare(rows)


def test_a_map_that_names_only_the_pooler_rows(block):
    rows = _map64([b * block.S for b in range(block.B)])
    assert int((rows >= 0).sum()) == block.B
    block.compare(rows)


def test_a_contraction_shorter_than_one_k_tile():
    """7 entries, B = 3 samples of 5 tokens, one head of 32, intermediate 40: the smallest the launcher takes."""
    small = _Block(3, 5, 32, 40, seed=7)
    small.compare(torch.tensor([0, 5, 10, 7, -1, 13, 2], dtype=torch.int32, device=DEV))


def test_two_mapped_backward_passes_give_bit_identical_parameter_gradients(block):
    from vilbert import _native
    rows = _map64([b * block.S for b in range(block.B)] + [151, 3, 36, 38, 73, 75, 110, 112, 184, 20])
    wanted = _native._DET["wanted"]
    _native.set_deterministic(True)
    try:
        dx0, g0 = block.run(rows, mapped=True)
        dx1, g1 = block.run(rows, mapped=True)
    finally:
        _native.set_deterministic(wanted)
    assert torch.equal(dx0, dx1)
    for n, g in g0.items():
        assert g.abs().max().item() > 0.0, n
        assert torch.equal(g, g1[n]), n
