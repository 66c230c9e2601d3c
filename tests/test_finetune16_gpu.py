"""The skinny-output linear of the fine-tuning heads (csrc/finetune16.hip, include/vilbert_hip_finetune.h) through vilbert.ops16:
forward, input gradient, weight + bias gradient against float64 arithmetic on the same bf16 inputs and fp32 weights.

The dropout mask is computed on the HOST (tests/dropout_restatement.py, pinned to csrc/rng.h by tests/test_dropout_mask.py) over the
element index r * K + k of the dense [rows, K] tensor - never read off a kernel. Bounds follow from the arithmetic (u = 2^-24, the
unit round-off of fp32):
  forward           fp32 products and an fp32 sum of K terms in any order: |err| <= 2 K u sum_k |drop(x) w|, plus one ulp of the
                    result (the additions of bias and row_add; row_add is 0 or -10000 as the region mask is)
  input gradient    one bf16 rounding (2^-9 relative, bound 2^-8) of scale * an fp32 sum of n terms, scale <= 2:
                    |err| <= 2^-8 |want| + n 2^-23 sum_j |dy w|; exactly +0 wherever the host mask drops
  weight gradient   an fp32 sum over the rows in a fixed order: |err| <= 2 rows u sum_r |dy drop(x)| (the survivors' scale is in
                    drop(x)); bias gradient: 2 rows u sum_r |dy|. Both onto a zero-filled target; onto a pre-filled target the
                    result is fl(old + that sum) bit for bit, and two runs agree bit for bit.
Rows 1, 7, 67, 300 (below one block of four waves, no multiple of any rows-per-block or rows-per-part, several blocks and parts),
K 8 .. 2048 (one active lane .. four chunks per lane), n 1 .. 4, row strides beyond the widths with sentinels in the gaps.

Last: the cast of a decoder's fp32 logit gradient with fp32 column sums (vbf_cast_rows_colsum) - the bf16 operand is torch's CPU
cast bit for bit with zero pad columns, the partial column sums are fp32 sums of at most 64 terms: |err| <= 64 u sum |x|."""
import numpy as np
import pytest
import torch

import dropout_restatement as DR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
U = 2.0 ** -24
SEED = 0xC0FFEE1234567891          # top bit set
ROWS = (1, 7, 67, 300)
KS = (8, 128, 768, 1024, 2048)
NS = (1, 2, 3, 4)
PS = (0.0, 0.1, 0.5)
SENT16, SENT32 = -7.0, -12345.0


@pytest.fixture(scope="module")
def ops16():
    import __graft_entry__
    __graft_entry__.build()
    from vilbert import ops16
    return ops16


def _case(rows, K, n, seed):
    """bf16-exact x, fp32 w / bias / dy (no zeros), row_add 0 or -10000: CPU tensors."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g).to(BF16)
    w = torch.randn(n, K, generator=g) * 0.05
    w = torch.where(w == 0, torch.full_like(w, 0.01), w)
    dy = torch.randn(rows, n, generator=g)
    dy = torch.where(dy == 0, torch.full_like(dy, 0.5), dy)
    bias = torch.randn(n, generator=g)
    row_add = torch.where(torch.rand(rows, generator=g) < 0.3, torch.tensor(-10000.0), torch.tensor(0.0))
    return x, w, bias, dy, row_add


def _strided(t, pad, sentinel):
    """t [rows, cols] on the device as a view of a [rows, cols + pad] buffer filled with `sentinel` -> (view, buffer)."""
    buf = torch.full((t.shape[0], t.shape[1] + pad), sentinel, dtype=t.dtype, device=DEV)
    buf[:, :t.shape[1]] = t.to(DEV)
    return buf[:, :t.shape[1]], buf


def _gap_untouched(buf, cols, sentinel):
    return bool((buf[:, cols:] == sentinel).all())


def _host_drop(x, p, seed, epoch=0):
    """(keep bool [rows, K], float64 drop(x)) with the host mask; p == 0 keeps everything at scale 1."""
    rows, K = x.shape
    if p == 0.0:
        return torch.ones(rows, K, dtype=torch.bool), x.double()
    keep = torch.from_numpy(DR.keep(DR.seed_with_epoch(seed, epoch), DR.linear_index(rows, K), p))
    scale = float(DR.drop_scale(p))
    return keep, torch.where(keep, x.double() * scale, torch.zeros((), dtype=torch.float64))


def _ulp32(v64):
    return torch.from_numpy(np.spacing(np.abs(v64.numpy()).astype(np.float32)).astype(np.float64))


def _check_all(ops16, rows, K, n, p, seed, epoch=0, report=None):
    x, w, bias, dy, row_add = _case(rows, K, n, seed=rows * 7919 + K * 31 + n)
    keep, xd = _host_drop(x, p, seed, epoch)
    scale = float(DR.drop_scale(p)) if p > 0 else 1.0
    xv, xbuf = _strided(x, 8, SENT16)
    dyv, dybuf = _strided(dy, 4, SENT32)
    wd, bd = w.to(DEV), bias.to(DEV)
    tag = "rows %d K %d n %d p %.1f" % (rows, K, n, p)

    # forward, with and without bias / row_add
    for with_extras in (True, False):
        ov, obuf = _strided(torch.zeros(rows, n), 3, SENT32)
        ops16.skinny_fwd(xv, wd, bd if with_extras else None, row_add.to(DEV) if with_extras else None, p, seed, out=ov)
        want = xd @ w.double().t()
        if with_extras:
            want = want + bias.double()[None, :] + row_add.double()[:, None]
        bound = 2 * K * U * (xd.abs() @ w.double().abs().t()) + _ulp32(want)
        err = (ov.cpu().double() - want).abs()
        assert (err <= bound).all(), "forward %s: worst err / bound %.3f" % (tag, float((err / bound).max()))
        assert _gap_untouched(obuf, n, SENT32) and _gap_untouched(xbuf, K, SENT16), tag
        if report is not None:
            report.append(float((err / bound).max()))

    # input gradient
    dv, dbuf = _strided(torch.zeros(rows, K, dtype=BF16), 16, SENT16)
    ops16.skinny_bwd_input(dyv, wd, p, seed, out=dv)
    got = dv.cpu()
    full = dy.double() @ w.double()
    want = torch.where(keep, full * scale, torch.zeros((), dtype=torch.float64))
    bound = want.abs() * 2.0 ** -8 + n * 2.0 ** -23 * (dy.double().abs() @ w.double().abs())
    err = (got.double() - want).abs()
    assert (err <= bound).all(), "input gradient %s: worst err / bound %.3f" % (tag, float((err / bound).max()))
    bits = got.view(torch.int16)
    assert bool((bits[~keep] == 0).all()), "input gradient %s: a dropped element is not +0" % tag
    if p > 0:      # nonzero dy and w: a survivor of the host mask that the kernel dropped would be a zero here
        assert bool((got[keep & (full.abs() > 1e-3)] != 0).all()), "input gradient %s: a survivor is zero" % tag
    assert _gap_untouched(dbuf, K, SENT16) and _gap_untouched(dybuf, n, SENT32), tag

    # weight and bias gradient: onto zeros (the bound), again (bit-identical), onto old content (fl(old + sum) bit for bit)
    (dw0,), (db0,) = ops16.skinny_bwd_weight(dyv, xv, n, True, drop_p=p, seed=seed)
    (dw1,), (db1,) = ops16.skinny_bwd_weight(dyv, xv, n, True, drop_p=p, seed=seed)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1), "weight gradient %s: two runs differ" % tag
    want_w, want_b = dy.double().t() @ xd, dy.double().sum(0)
    bound_w = 2 * rows * U * (dy.double().abs().t() @ xd.abs())
    bound_b = 2 * rows * U * dy.double().abs().sum(0)
    err_w, err_b = (dw0.cpu().double() - want_w).abs(), (db0.cpu().double() - want_b).abs()
    assert (err_w <= bound_w).all(), "weight gradient %s: worst err / bound %.3f" % (tag, float((err_w / bound_w.clamp_min(1e-300)).max()))
    assert (err_b <= bound_b).all(), "bias gradient %s: worst err / bound %.3f" % (tag, float((err_b / bound_b).max()))
    g = torch.Generator().manual_seed(5)
    old_w, old_b = torch.randn(n, K, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
    tw, tb = old_w.clone(), old_b.clone()
    ops16.skinny_bwd_weight(dyv, xv, n, True, dw_out=tw, db_out=tb, drop_p=p, seed=seed)
    assert torch.equal(tw, old_w + dw0) and torch.equal(tb, old_b + db0), "weight gradient %s: not added into the target" % tag
    assert not torch.equal(tw, dw0)
    # without a bias gradient the weight gradient is the same
    (dw2,), (db2,) = ops16.skinny_bwd_weight(dyv, xv, n, False, drop_p=p, seed=seed)
    assert db2 is None and torch.equal(dw2, dw0), tag
    assert _gap_untouched(xbuf, K, SENT16) and _gap_untouched(dybuf, n, SENT32), tag


def test_shapes_the_kernels_serve(ops16):
    assert ops16.skinny_ok(768, 1) and ops16.skinny_ok(1024, 1) and ops16.skinny_ok(8, 4) and ops16.skinny_ok(2048, 4)
    assert not ops16.skinny_ok(2056, 1) and not ops16.skinny_ok(12, 1) and not ops16.skinny_ok(0, 1)
    assert not ops16.skinny_ok(768, 0) and not ops16.skinny_ok(768, 5)
    with pytest.raises(RuntimeError):
        ops16.skinny_fwd(torch.zeros(4, 2056, dtype=BF16, device=DEV), torch.zeros(1, 2056, device=DEV))
    with pytest.raises(RuntimeError):      # no CPU fallback
        ops16.skinny_fwd(torch.zeros(4, 64, dtype=BF16), torch.zeros(1, 64, device=DEV))


@pytest.mark.parametrize("K", KS)
def test_forward_and_gradients_against_float64_with_the_host_mask(ops16, K):
    worst = []
    for rows in ROWS:
        for n in NS:
            for p in PS:
                _check_all(ops16, rows, K, n, p, SEED + rows + n, report=worst)
    torch.cuda.synchronize()
    print("skinny linear K = %d: worst forward err / bound %.3f over %d launches" % (K, max(worst), len(worst)))


def test_the_mask_does_not_depend_on_the_row_stride_and_differs_between_seeds(ops16):
    rows, K, n, p = 67, 128, 2, 0.5
    x, w, _b, dy, _a = _case(rows, K, n, seed=3)
    xv, _ = _strided(x, 24, SENT16)
    dense = ops16.skinny_bwd_input(dy.to(DEV), w.to(DEV), p, SEED)
    other = ops16.skinny_bwd_input(dy.to(DEV), w.to(DEV), p, SEED + 1)
    assert not torch.equal(dense == 0, other == 0)
    a = ops16.skinny_fwd(xv, w.to(DEV), None, None, p, SEED)
    b = ops16.skinny_fwd(x.to(DEV), w.to(DEV), None, None, p, SEED)
    assert torch.equal(a, b)
    # p == 0 ignores the seed
    assert torch.equal(ops16.skinny_fwd(xv, w.to(DEV), None, None, 0.0, 1), ops16.skinny_fwd(xv, w.to(DEV), None, None, 0.0, 2))


def test_registered_step_counter_is_mixed_into_the_seed(ops16):
    from vilbert import _native as N
    from vilbert import graphed
    epoch = 5
    counter = torch.tensor([epoch], dtype=torch.int64, device=DEV)      # one 64-bit word: the uint64 the kernels read
    before = graphed._ACTIVE["epoch_ptr"]                              # a GraphedTrainStep that is still alive, if any
    rows, K = 67, 768
    x = _case(rows, K, 1, seed=rows * 7919 + K * 31 + 1)[0]
    assert not torch.equal(_host_drop(x, 0.5, SEED, 0)[0], _host_drop(x, 0.5, SEED, epoch)[0])
    N.check(N.lib().vb_set_seed_epoch(counter.data_ptr()), "vb_set_seed_epoch")
    try:
        _check_all(ops16, rows, K, 1, 0.5, SEED, epoch=epoch)
        _check_all(ops16, 7, 128, 3, 0.1, SEED, epoch=epoch)
        torch.cuda.synchronize()
    finally:
        N.lib().vb_set_seed_epoch(before)


def test_a_nan_stays_in_its_row(ops16):
    rows, K, n = 67, 768, 3
    x, w, bias, _dy, row_add = _case(rows, K, n, seed=11)
    clean = ops16.skinny_fwd(x.to(DEV), w.to(DEV), bias.to(DEV), row_add.to(DEV)).cpu()
    x[41, 700] = float("nan")
    got = ops16.skinny_fwd(x.to(DEV), w.to(DEV), bias.to(DEV), row_add.to(DEV)).cpu()
    assert torch.isnan(got[41]).all()
    others = torch.arange(rows) != 41
    assert torch.isfinite(got[others]).all() and torch.equal(got[others], clean[others])


@pytest.mark.parametrize("rows,n", [(1, 3), (67, 211), (300, 1601), (130, 256)])
def test_cast_rows_with_column_sums(ops16, rows, n):
    g = torch.Generator().manual_seed(rows + n)
    n_pad = (n + 255) // 256 * 256
    x = torch.randn(rows, n, generator=g)
    xv, xbuf = _strided(x, 4 + (-n) % 4, SENT32)                       # row stride % 4 == 0, beyond n
    assert xv.stride(0) % 4 == 0 and xv.stride(0) > n
    G, part = ops16.cast_rows_colsum(xv)
    torch.cuda.synchronize()
    assert G.shape == (rows, n_pad) and part.shape == ((rows + 63) // 64, n_pad)
    assert torch.equal(G[:, :n].cpu().view(torch.int16), x.to(BF16).view(torch.int16)) and not G[:, n:].any()
    assert _gap_untouched(xbuf, n, SENT32)
    pad = torch.zeros((rows + 63) // 64 * 64 - rows, n)
    blocks = torch.cat([x, pad]).double().view(-1, 64, n)
    want, mag = blocks.sum(1), blocks.abs().sum(1)
    err = (part[:, :n].cpu().double() - want).abs()
    assert (err <= 64 * U * mag).all(), float((err / (64 * U * mag).clamp_min(1e-300)).max())
    assert not part[:, n:].any()
    # the ordered sum of the partial rows is the column sum, added into its target
    old = torch.randn(n, generator=g).to(DEV)
    out = ops16.colsum_parts(part, n, old.clone())
    err = (out.cpu().double() - old.cpu().double() - x.double().sum(0)).abs()
    assert (err <= (rows + 1) * U * (x.double().abs().sum(0) + old.cpu().double().abs())).all()
    G2, part2 = ops16.cast_rows_colsum(xv)
    assert torch.equal(G, G2) and torch.equal(part, part2)
