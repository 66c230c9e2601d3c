"""Device-side MLM and region masking on the GPU (csrc/mask_batch.hip, vilbert.input_pipeline.mask_batch / DeviceBatchPipeline
with masking=...): every output equals the numpy restatement (tests/masking_restatement.py) EXACTLY - the work is integer
arithmetic, comparisons of exactly representable fp32 values, one correctly rounded fp32 division, copies and zeros, so there is
no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest
import torch

import masking_restatement as mr
from oracle import batch_oracle as bo

pytestmark = pytest.mark.gpu
VOCAB, MASK_ID = 30522, 103
MASK_OUT = ("input_ids", "lm_label_ids", "image_label", "masked_label", "image_feat")


def _to_dev(raw):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in raw.items()}


def _same(a, b, name):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (name, a.shape, b.shape, a.dtype, b.dtype)
    assert np.array_equal(a, b), name


def _check_mask(raw, seed, p, inplace):
    from vilbert import input_pipeline as ip
    want = mr.mask_batch(raw, seed, VOCAB, MASK_ID, p)
    dev = _to_dev(raw)
    got = ip.mask_batch(dev, seed, VOCAB, MASK_ID, p, inplace=inplace)
    assert sorted(got) == sorted(ip.RAW_FIELDS)
    for n in ip.RAW_FIELDS:
        _same(got[n].cpu().numpy(), want[n], n)
    assert got["image_target"] is dev["image_target"]
    if inplace:
        assert got["input_ids"] is dev["input_ids"] and got["image_feat"] is dev["image_feat"]
    else:
        for n in mr.RAW_UNMASKED_FIELDS:                        # the unmasked batch is left as it was
            _same(dev[n].cpu().numpy(), raw[n], "input " + n)
    return want


@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "copy"])
@pytest.mark.parametrize("shape", [(3, 12, 7, 64), (5, 36, 37, 2048), (1, 9, 5, 8), (2, 70, 130, 8)],
                         ids=lambda s: "B%d-T%d-R%d-F%d" % s)
def test_kernels_equal_the_restatement_exactly(shape, inplace):
    """(2, 70, 130, 8): more tokens and regions than one wave holds, the second and third 64-region chunks of the OR."""
    B, T, R, F = shape
    raw = mr.make_unmasked_batch(B, tokens=T, regions=R, feat_dim=F, n_classes=5, vocab=VOCAB, seed=B + T)
    want = _check_mask(raw, 0xC0FFEE + B, 0.15 if B != 2 else 0.3, inplace)
    if B >= 3:
        assert (want["lm_label_ids"] != -1).any() and (want["image_label"] == 1).any()      # the case selects something


@pytest.mark.parametrize("p", [0.0, 0.15, 1.0])
def test_edge_samples(p):
    """len = 2 (no eligible token), len = 0, 1, 3 and T; no box, one box and all R boxes; p_select 0 and 1; overlaps holding
    entries exactly at 0.4 (make_unmasked_batch places them: they must not mask, their upper neighbours must)."""
    raw = mr.make_unmasked_batch(6, tokens=12, regions=7, feat_dim=8, n_classes=3, vocab=VOCAB, seed=1,
                                 n_tok=[2, 3, 12, 0, 1, 7], n_box=[0, 7, 1, 3, 7, 0])
    assert (raw["overlaps"] == np.float32(0.4)).sum() >= 3
    want = _check_mask(raw, 9, p, False)
    if p == 1.0:
        assert [(r != -1).sum() for r in want["lm_label_ids"]] == [0, 1, 10, 0, 0, 5]
        assert [(r == 1).sum() for r in want["image_label"]] == [0, 7, 1, 3, 7, 0]
    if p == 0.0:
        assert (want["lm_label_ids"] == -1).all() and (want["masked_label"] == 0).all()


def test_threshold_entries_alone_do_not_mask():
    from vilbert import input_pipeline as ip
    raw = mr.make_unmasked_batch(1, tokens=4, regions=3, feat_dim=4, n_classes=2, vocab=VOCAB, seed=0, n_tok=[4], n_box=[1])
    raw["overlaps"][:] = 0
    raw["overlaps"][0, 0] = [1.0, 0.4, np.nextafter(np.float32(0.4), np.float32(1))]
    got = ip.mask_batch(_to_dev(raw), 3, VOCAB, MASK_ID, 1.0, inplace=False)
    assert got["image_label"].tolist() == [[1, -1, -1]] and got["masked_label"].tolist() == [[1, 0, 1]]


def test_same_inputs_same_bits_and_seeds_matter():
    from vilbert import input_pipeline as ip
    raw = mr.make_unmasked_batch(8, tokens=36, regions=36, feat_dim=16, n_classes=3, vocab=VOCAB, seed=5)
    dev = _to_dev(raw)
    a, b = (ip.mask_batch(dev, 11, VOCAB, MASK_ID, inplace=False) for _ in range(2))
    c = ip.mask_batch(dev, 12, VOCAB, MASK_ID, inplace=False)
    for n in MASK_OUT:
        assert torch.equal(a[n], b[n]), n
    assert not torch.equal(a["lm_label_ids"], c["lm_label_ids"]) and not torch.equal(a["image_label"], c["image_label"])


# ---- vbi_zero_rows ---------------------------------------------------------------------------------------------------------------
def _padded(rows, n, ld, margin, seed):
    """A flat buffer: canary margin | rows x ld (random data in the first n columns, NaN in the gap) | canary margin."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.full((2 * margin + rows * ld,), 7.25)
    body = flat[margin:margin + rows * ld].view(rows, ld)
    body[:, :n] = torch.randn(rows, n, generator=g)
    body[:, n:] = float("nan")
    return flat


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("rows,n,ld", [(5, 64, 72), (2500, 8, 12), (3, 2052, 2056), (1, 4, 4)],
                         ids=["small", "grid-stride", "wide-row", "one-chunk"])
def test_zero_rows_in_place_and_out_of_place(rows, n, ld):
    """Canary margins, strided rows, NaN between n and the row stride; more rows than the grid has blocks; a row wider than one
    pass of the block. Unflagged rows, the gaps and the margins keep their bits."""
    from vilbert import _native as N
    margin = 64
    host = _padded(rows, n, ld, margin, 1)
    flags = (torch.rand(rows, generator=torch.Generator().manual_seed(2)) < 0.4)
    flags[0], flags[-1] = True, rows == 1
    want = host.clone()
    want[margin:margin + rows * ld].view(rows, ld)[flags, :n] = 0
    fl = flags.to(torch.uint8).cuda()
    # in place
    x = host.cuda()
    xp = x.data_ptr() + 4 * margin
    N.check(N.lib().vbi_zero_rows(N.stream_ptr(), rows, n, xp, ld, fl.data_ptr(), None, 0), "vbi_zero_rows")
    assert torch.equal(_bits(x), _bits(want))
    # out of place, into a buffer with another stride
    ldo = ld + 4
    x = host.cuda()
    out_host = _padded(rows, n, ldo, margin, 3)
    out = out_host.cuda()
    N.check(N.lib().vbi_zero_rows(N.stream_ptr(), rows, n, x.data_ptr() + 4 * margin, ld, fl.data_ptr(),
                                  out.data_ptr() + 4 * margin, ldo), "vbi_zero_rows")
    want_out = out_host.clone()
    want_out[margin:margin + rows * ldo].view(rows, ldo)[:, :n] = want[margin:margin + rows * ld].view(rows, ld)[:, :n]
    assert torch.equal(_bits(out), _bits(want_out))
    assert torch.equal(_bits(x), _bits(host))                   # the source is only read


def test_zero_rows_alignment_errors_write_nothing():
    from vilbert import _native as N
    rows, n, ld, margin = 4, 8, 8, 16
    host = _padded(rows, n, ld, margin, 4)
    x, out = host.cuda(), host.cuda()
    fl = torch.ones(rows, dtype=torch.uint8).cuda()
    xp, op = x.data_ptr() + 4 * margin, out.data_ptr() + 4 * margin
    zr, st = N.lib().vbi_zero_rows, N.stream_ptr()
    assert zr(st, rows, n, xp + 4, ld, fl.data_ptr(), None, 0) == -2           # x off by one float
    assert zr(st, rows, 6, xp, ld, fl.data_ptr(), None, 0) == -2               # n % 4
    assert zr(st, rows, n, xp, 10, fl.data_ptr(), None, 0) == -2               # row stride % 4
    assert zr(st, rows, n, xp, ld, fl.data_ptr(), op + 8, ld) == -2            # out off by two floats
    assert zr(st, rows, n, xp, ld, fl.data_ptr(), op, 9) == -2
    assert zr(st, rows, n, xp, ld, fl.data_ptr(), xp, ld) == -1                # out == x
    torch.cuda.synchronize()
    assert torch.equal(_bits(x), _bits(host)) and torch.equal(_bits(out), _bits(host))
    with pytest.raises(RuntimeError, match="vbi_zero_rows failed"):
        N.check(zr(st, rows, 6, xp, ld, fl.data_ptr(), None, 0), "vbi_zero_rows")


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
def _unmasked_source(n):
    raws = [mr.make_unmasked_batch(4 + (i % 2), tokens=10, regions=6, feat_dim=64, n_classes=9, vocab=99, seed=40 + i)
            for i in range(n)]
    source = [tuple(r[f] if f != "input_ids" else r[f].astype(np.int32) for f in mr.RAW_UNMASKED_FIELDS) + (["id%d" % i],)
              for i, r in enumerate(raws)]
    return raws, source


@pytest.mark.parametrize("objective", [0, 1])
def test_masking_pipeline_equals_finish_batch_of_the_restated_masked_batch(objective):
    from vilbert import input_pipeline as ip
    raws, source = _unmasked_source(3)
    masking = ip.Masking(seed=2024, vocab_size=99, mask_token_id=3, p_select=0.3, first_batch=2)
    seen = 0
    for i, batch in enumerate(ip.DeviceBatchPipeline(source, "cuda:0", objective=objective, masking=masking)):
        assert len(batch) == 11 and batch[10] == ["id%d" % i]
        masked = mr.mask_batch(raws[i], mr.batch_seed(2024, 2 + i), 99, 3, 0.3)
        assert (masked["lm_label_ids"] != -1).any() and (masked["image_label"] == 1).any()
        want = bo.finish_batch(masked, objective)
        got = [t.cpu().numpy() for t in batch[:10]]      # read before the slot is reused
        for j, n in enumerate(bo.OUT_FIELDS):
            _same(got[j], want[n], "batch %d %s" % (i, n))
        torch.cuda.current_stream().synchronize()
        seen += 1
    assert seen == 3


def _run_pipeline(pipe):
    out = []
    for batch in pipe:
        out.append([t.cpu().numpy() for t in batch[:10]])      # read before the slot is reused
        torch.cuda.current_stream().synchronize()
    return out


def test_every_pass_draws_new_masks_and_a_restart_repeats_them():
    """The Masking object counts batches across iterations: pass 2 over the same three batches uses global batches 3, 4, 5 - other
    masks than pass 1, each equal to the restatement at its global index; a second pipeline that shares the object goes on
    counting; a run restarted with first_batch=k repeats global batch k. The label slots of the source are never read."""
    from vilbert import input_pipeline as ip
    raws, source = _unmasked_source(3)
    lm_slot, il_slot = (mr.RAW_UNMASKED_FIELDS.index(n) for n in ("lm_label_ids", "image_label"))
    source = [tuple(np.full_like(x, 77) if k in (lm_slot, il_slot) else x for k, x in enumerate(b)) for b in source]
    masking = ip.Masking(seed=31, vocab_size=99, mask_token_id=3, p_select=0.3)
    pipe = ip.DeviceBatchPipeline(source, "cuda:0", objective=0, masking=masking)
    passes = [_run_pipeline(pipe), _run_pipeline(pipe)]
    passes.append(_run_pipeline(ip.DeviceBatchPipeline(source, "cuda:0", objective=0, masking=masking)))
    assert masking.next_batch == 9 and masking.first_batch == 0
    for p, got in enumerate(passes):
        assert len(got) == 3
        for i in range(3):
            want = bo.finish_batch(mr.mask_batch(raws[i], mr.batch_seed(31, 3 * p + i), 99, 3, 0.3), 0)
            for j, n in enumerate(bo.OUT_FIELDS):
                _same(got[i][j], want[n], "pass %d batch %d %s" % (p, i, n))
    lm, il = bo.OUT_FIELDS.index("lm_label_ids"), bo.OUT_FIELDS.index("image_label")
    for p, q in ((0, 1), (0, 2), (1, 2)):
        for i in range(3):
            assert not np.array_equal(passes[p][i][lm], passes[q][i][lm]), (p, q, i)
            assert not np.array_equal(passes[p][i][il], passes[q][i][il]), (p, q, i)
    # restarted at global batch 4 = batch 1 of pass 2, fed that batch's sample
    again = _run_pipeline(ip.DeviceBatchPipeline(source[1:], "cuda:0", objective=0,
                                                 masking=ip.Masking(31, 99, 3, p_select=0.3, first_batch=4)))
    for k in range(2):
        for j, n in enumerate(bo.OUT_FIELDS):
            _same(again[k][j], passes[1][1 + k][j], "restart batch %d %s" % (4 + k, n))


def test_default_pipeline_is_unchanged():
    """masking=None: the masked source of tests/test_input_pipeline.py, finished as before (the oracle that the parent's kernels
    equal bit for bit), whether the argument is left out or passed."""
    from vilbert import input_pipeline as ip
    raws = [bo.make_raw_batch(4 + (i % 2), tokens=10, regions=6, feat_dim=64, n_classes=9, vocab=99, seed=30 + i) for i in range(3)]
    source = [tuple(r[n] for n in bo.RAW_FIELDS) + (i,) for i, r in enumerate(raws)]
    for kwargs in ({}, {"masking": None}):
        pipe = ip.DeviceBatchPipeline(source, "cuda:0", objective=1, **kwargs)
        assert pipe.masking is None and pipe.fields == ip.RAW_FIELDS == bo.RAW_FIELDS
        for i, batch in enumerate(pipe):
            want = bo.finish_batch(raws[i], 1)
            assert len(batch) == 11 and batch[10] == i
            for j, n in enumerate(bo.OUT_FIELDS):
                _same(batch[j].cpu().numpy(), want[n], "batch %d %s" % (i, n))
            torch.cuda.current_stream().synchronize()


def test_graph_replay_gives_the_eager_bits():
    from vilbert import input_pipeline as ip
    raw = mr.make_unmasked_batch(5, tokens=36, regions=37, feat_dim=64, n_classes=3, vocab=VOCAB, seed=8)
    dev = _to_dev(raw)
    eager = ip.mask_batch(dev, 21, VOCAB, MASK_ID, inplace=False)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ip.mask_batch(dev, 21, VOCAB, MASK_ID, inplace=False)          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ip.mask_batch(dev, 21, VOCAB, MASK_ID, inplace=False)
    for n in MASK_OUT:
        captured[n].fill_(-7)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for n in MASK_OUT:
        assert torch.equal(captured[n], eager[n]), n
    want = mr.mask_batch(raw, 21, VOCAB, MASK_ID)
    for n in MASK_OUT:
        _same(captured[n].cpu().numpy(), want[n], n)
