"""Row lists of the last encoder layers in a pre-training step (vilbert.BertForMultiModalPreTraining: _static_label_rows +
_row_map), in plain torch on the CPU.

The last text / image layer computes its output + feed-forward block only on a compact row list: row 0 of every sample (the
poolers), then the fixed-capacity labelled rows (the prediction heads), -1 for padding and for a labelled row 0 (it is in the
list already: the head reads the pooler entry, so every row is computed once). Emulating that compact output from a random
full hidden state, the rows and labels the heads see must be the ones the exact gather (torch.nonzero) selects."""
import pytest
import torch

from oracle import synth

B, T, R, H = 4, 6, 5, 8         # samples, tokens, regions without the global row, hidden size


def _model():
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    return BertForMultiModalPreTraining(BertConfig.from_dict(synth.tiny_config()))


def _labels():
    lm = torch.full((B, T), -1, dtype=torch.int64)
    lm[0, 0], lm[0, 3] = 11, 12         # token 0 labelled next to another token: that row is a pooler row AND a labelled row
    lm[1, 0] = 13                       # token 0 is the sample's only label
    lm[3, 2], lm[3, 5] = 14, 15         # (sample 2: no label at all)
    il = torch.zeros((B, R), dtype=torch.int64)
    il[0, 0], il[0, 4], il[2, 1], il[3, 3] = 1, 1, 1, 1
    return lm, il


def _compact(full, row_map):
    idx = row_map.to(torch.int64)
    return full.index_select(0, idx.clamp(min=0)) * (idx >= 0).unsqueeze(1).to(full.dtype)


def _check(cap, monkeypatch):
    import vilbert.vilbert as V
    lm, il = _labels()
    if cap is not None:
        monkeypatch.setattr(V, "_capacity", lambda positions, frac: cap)
    m = _model()
    m.label_capacity = 0.5
    idx_t, labels_t, idx_r, valid_r, _div, n_t, n_r = m._static_label_rows(lm, il)
    idx_v = idx_r + torch.div(idx_r, R, rounding_mode="floor") + 1
    (map_t, head_t), (map_v, head_v) = V._row_map(idx_t, n_t, B, T), V._row_map(idx_v, n_r, B, R + 1)
    g = torch.Generator().manual_seed(1)
    full_t, full_v = torch.randn(B * T, H, generator=g), torch.randn(B * (R + 1), H, generator=g)

    exact_t = torch.nonzero(lm.reshape(-1) != -1).squeeze(1)
    with_global = torch.cat([torch.zeros(B, 1, dtype=il.dtype), il], dim=1)            # labels inside [B, R + 1]
    exact_v = torch.nonzero(with_global.reshape(-1) == 1).squeeze(1)
    for row_map, head_idx, full, exact, per, cap_n in ((map_t, head_t, full_t, exact_t, T, idx_t.numel()),
                                                       (map_v, head_v, full_v, exact_v, R + 1, idx_r.numel())):
        assert row_map.dtype == torch.int32 and row_map.numel() % 32 == 0 and row_map.numel() >= B + cap_n
        named = row_map[row_map >= 0]
        assert named.unique().numel() == named.numel()                                   # every row once
        out = _compact(full, row_map)
        assert torch.equal(out[:B], full[torch.arange(B) * per])                         # what the poolers read
        used = min(exact.numel(), cap_n)
        assert head_idx.shape == (cap_n,)
        head = out.index_select(0, head_idx)
        assert torch.equal(head[:used], full[exact[:used]])                              # what the heads read
        assert torch.equal(row_map[B + used:], torch.full_like(row_map[B + used:], -1))  # padding: nothing scattered back
        assert not head[used:].any()
    used_t, used_r = min(exact_t.numel(), idx_t.numel()), min(exact_v.numel(), idx_r.numel())
    assert torch.equal(labels_t[:used_t], lm.reshape(-1)[exact_t[:used_t]]) and (labels_t[used_t:] == -1).all()
    assert valid_r[:used_r].all() and not valid_r[used_r:].any()
    assert head_t[:used_t].tolist() == [{0: 0, T: 1}.get(r, B + i) for i, r in enumerate(exact_t[:used_t].tolist())]
    return m, map_t, exact_t, exact_v


def test_rows_and_labels_equal_the_exact_gather_with_padding(monkeypatch):
    m, map_t, exact_t, _ = _check(None, monkeypatch)                 # capacity 32: 5 tokens / 4 regions + padding
    m.check_label_capacity()
    # token 0 of samples 0 and 1: pooler row and labelled row at once - in the map once, the head reads the pooler entry
    assert exact_t.tolist() == [0, 3, T, 3 * T + 2, 3 * T + 5]
    assert (map_t == 0).sum() == 1 and (map_t == T).sum() == 1
    assert map_t[B:B + 5].tolist() == [-1, 3, -1, 3 * T + 2, 3 * T + 5]


def test_exactly_full_capacity(monkeypatch):
    m, _, _, _ = _check(5, monkeypatch)                              # 5 labelled tokens fill it; 4 regions leave one padding row
    m.check_label_capacity()


def test_capacity_overflow_keeps_the_first_rows_and_is_reported(monkeypatch):
    m, map_t, exact_t, exact_v = _check(3, monkeypatch)
    assert exact_t.numel() > 3 and exact_v.numel() > 3
    assert map_t[B:B + 3].tolist() == [-1, 3, -1]            # (rows 0 and T: the pooler entries)
    with pytest.raises(RuntimeError, match="capacity"):
        m.check_label_capacity()
