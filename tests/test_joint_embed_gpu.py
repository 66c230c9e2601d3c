"""Direct C-ABI tests of the kernels of the single-stream baseline (csrc/joint_embed.hip, include/vilbert_hip_baseline.h): the
joint text + image embedding, its backward, the table scatter with padding rows and the pooler's tanh, on guarded buffers
against float64 restatements. Tolerances are those of the direct row-kernel tests (tests/test_row_kernels_abi_gpu.py,
tests/row_kernel_bounds.py): the kernels share rowops.h's LayerNorm finish and layernorm.hip's backward arithmetic.

Shapes (B, T, R, H): the degenerate minimum; 4-row blocks that straddle the segment and the sample boundary (12 rows per
sample); the base and large widths and a ragged last 256-column chunk (1028: also the one-partial-per-row backward); 300 rows
(more than 16 partials in a segment, so stage 2 of the column sums adds more than one part per group); the real joint length."""
import pytest
import torch

import row_kernel_bounds as RB
from test_row_kernels_abi_gpu import DEV, NAN, U, Guard, _bits, _close, _lib, _N, _st, _within

pytestmark = pytest.mark.gpu
I64 = torch.int64
VOCAB, N_TYPES = 11, 2
SHAPES = [(1, 1, 1, 4), (3, 7, 5, 64), (3, 7, 5, 96), (3, 7, 5, 768), (3, 7, 5, 1024), (3, 7, 5, 1028), (25, 7, 5, 768),
          (2, 38, 101, 768)]


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _ln_params(cols, seed):
    g = torch.Generator().manual_seed(seed)
    return 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)


def _inputs(B, T, R, H, seed=0):
    """Everything one forward reads, as CPU tensors; a few ids lie outside their tables."""
    gen = torch.Generator().manual_seed(1000 * seed + H + T)
    ids = torch.randint(0, VOCAB, (B, T), generator=gen)
    seg = torch.randint(0, N_TYPES, (B, T), generator=gen)
    if T >= 7:
        ids[0, 1], ids[B - 1, 2], ids[B - 1, 6] = VOCAB + 5, -3, VOCAB
        seg[0, 3] = N_TYPES
    x = dict(ids=ids, seg=seg, word=_rand(VOCAB, H, seed=1), pos=_rand(T, H, seed=2), typ=_rand(N_TYPES, H, seed=3),
             proj=_rand(B, R, H, seed=4), loc=torch.rand(B, R, 5, generator=gen), wl=_rand(H, 5, seed=5), bl=_rand(H, seed=6),
             trow=_rand(H, seed=7))
    x["gt"], x["bt"] = _ln_params(H, 8)
    x["gv"], x["bv"] = _ln_params(H, 9)
    x["mask_t"] = torch.randint(0, 2, (B, T), generator=gen)
    x["mask_v"] = torch.randint(0, 2, (B, R), generator=gen)
    return x


def _joint_fwd(x, mask_t=None, mask_v=None, eps=1e-12, want=True):
    """One vbb_joint_embed_fwd launch, every operand in a guarded buffer of exactly its size -> CPU out [B, S, H], mean [B, S],
    rstd [B, S], presum [B, S, H], add_mask [B, S] (mean / rstd / presum None without `want`)."""
    B, T = x["ids"].shape
    R, H = x["proj"].shape[1], x["proj"].shape[2]
    S = T + R
    g = {k: Guard.of(x[k]) for k in ("ids", "seg", "word", "pos", "typ", "gt", "bt", "proj", "loc", "wl", "bl", "trow", "gv", "bv")}
    mt = Guard.of(mask_t) if mask_t is not None else None
    mv = Guard.of(mask_v) if mask_v is not None else None
    out, add = Guard(B * S * H), Guard(B * S)
    mean, rstd, presum = (Guard(B * S), Guard(B * S), Guard(B * S * H)) if want else (None, None, None)
    rc = _lib().vbb_joint_embed_fwd(
        _st(), B, T, R, H, VOCAB, N_TYPES, g["ids"].ptr, g["seg"].ptr, g["word"].ptr, g["pos"].ptr, g["typ"].ptr, g["gt"].ptr,
        g["bt"].ptr, g["proj"].ptr, g["loc"].ptr, g["wl"].ptr, g["bl"].ptr, g["trow"].ptr, g["gv"].ptr, g["bv"].ptr, eps,
        mt.ptr if mt else None, int(mask_t is not None and mask_t.dtype == torch.float32),
        mv.ptr if mv else None, int(mask_v is not None and mask_v.dtype == torch.float32),
        out.ptr, mean.ptr if want else None, rstd.ptr if want else None, presum.ptr if want else None, add.ptr)
    assert rc == 0, rc
    what = "vbb_joint_embed_fwd %s" % ((B, T, R, H),)
    return (out.cpu(what).view(B, S, H), mean.cpu(what).view(B, S) if want else None, rstd.cpu(what).view(B, S) if want else None,
            presum.cpu(what).view(B, S, H) if want else None, add.cpu(what).view(B, S))


def _presum64(x):
    """float64 pre-LayerNorm sums of the two segments and the sums of their |terms| (ids outside their table: zero rows)."""
    B, T = x["ids"].shape

    def rows_of(table, idx):
        ok = ((idx >= 0) & (idx < table.shape[0])).double()[..., None]
        return table.double()[idx.clamp(0, table.shape[0] - 1)] * ok

    w, t = rows_of(x["word"], x["ids"]), rows_of(x["typ"], x["seg"])
    p = x["pos"].double()[None, :T].expand(B, -1, -1)
    terms = x["loc"].double()[:, :, None, :] * x["wl"].double()[None, None, :, :]          # [B, R, H, 5]
    tr, bl = x["trow"].double(), x["bl"].double()
    e_v = x["proj"].double() + tr + terms.sum(-1) + bl
    mag_v = x["proj"].double().abs() + tr.abs() + terms.abs().sum(-1) + bl.abs()
    return (w + p + t, w.abs() + p.abs() + t.abs()), (e_v, mag_v)


@pytest.mark.parametrize("B,T,R,H", SHAPES)
def test_joint_embedding_out_statistics_presum_and_both_mask_types(B, T, R, H):
    x = _inputs(B, T, R, H)
    out, mean, rstd, presum, add = _joint_fwd(x, x["mask_t"], x["mask_v"].float())
    (e_t, mag_t), (e_v, mag_v) = _presum64(x)
    what = "%s" % ((B, T, R, H),)
    _within(presum[:, :T], e_t, 3 * U * mag_t + 1e-37, what + " text presum")             # two fp32 additions
    _within(presum[:, T:], e_v, 9 * U * mag_v + 1e-37, what + " image presum")            # five fused multiply-adds, three additions
    for sl, e64, g, b, name in ((slice(0, T), e_t, x["gt"], x["bt"], "text"), (slice(T, T + R), e_v, x["gv"], x["bv"], "image")):
        ref = RB.ln64(e64.reshape(-1, H), g, b, 1e-12)
        _close(out[:, sl].reshape(-1, H), ref["y"], what=what + " %s out" % name)
        _close(mean[:, sl].reshape(-1), ref["mean"], what=what + " %s mean" % name)
        _close(rstd[:, sl].reshape(-1), ref["rstd"], 1e-5, 1e-6, what=what + " %s rstd" % name)
    want_mask = torch.cat([(1.0 - x["mask_t"].float()) * -10000.0, (1.0 - x["mask_v"].float()) * -10000.0], 1)
    assert torch.equal(add, want_mask)
    # the other mask types, no statistics wanted: the same rows bit for bit, the mask exact
    out2, _, _, _, add2 = _joint_fwd(x, x["mask_t"].float(), x["mask_v"], want=False)
    assert torch.equal(_bits(out2), _bits(out)) and torch.equal(add2, want_mask)
    out3, _, _, _, add3 = _joint_fwd(x, None, None, want=False)
    # (a NULL mask is an all-ones mask: (1 - 1) * -10000, the same -0.0)
    assert torch.equal(_bits(out3), _bits(out)) and torch.equal(_bits(add3), _bits((1.0 - torch.ones(B, T + R)) * -10000.0))


def test_an_id_outside_its_table_gives_a_zero_row():
    B, T, R, H = 2, 3, 2, 64
    x = _inputs(B, T, R, H)
    x["pos"].zero_()
    x["ids"][0, 1], x["ids"][1, 2] = VOCAB, -1
    x["seg"][0, 1], x["seg"][1, 2] = N_TYPES, -1
    out, mean, rstd, presum, _ = _joint_fwd(x)
    for b, j in ((0, 1), (1, 2)):
        assert float(presum[b, j].abs().max()) == 0.0
        assert torch.equal(out[b, j], x["bt"]) and float(mean[b, j]) == 0.0            # a constant row: its LayerNorm is beta
    assert float(presum[0, 0].abs().max()) > 0.0


def test_a_nan_poisons_its_row_only():
    B, T, R, H = 3, 7, 5, 768
    x = _inputs(B, T, R, H)
    x["ids"] = torch.randint(1, VOCAB, (B, T), generator=torch.Generator().manual_seed(3))
    x["ids"][1, 4] = 0
    x["word"][0, 300] = NAN                                                # id 0 appears at (1, 4) only
    x["proj"][2, 3, 5] = NAN
    out, mean, rstd, presum, add = _joint_fwd(x, x["mask_t"], x["mask_v"])
    bad = torch.zeros(B, T + R, dtype=torch.bool)
    bad[1, 4] = bad[2, T + 3] = True
    assert torch.equal(torch.isnan(out).all(-1), bad) and torch.equal(torch.isnan(out).any(-1), bad)
    assert torch.equal(torch.isnan(mean), bad) and torch.equal(torch.isnan(rstd), bad)
    assert torch.isfinite(add).all()


def _joint_bwd(B, T, R, H, dy, x, mean, rstd, gt, gv):
    """One vbb_joint_embed_bwd launch on a NaN-filled workspace of exactly vbb_joint_embed_bwd_workspace floats and NaN-filled
    column sums -> CPU dx_text [B * T, H], dx_img [B * R, H], dgamma_t, dbeta_t, dgamma_v, dbeta_v."""
    lib = _lib()
    ws_n = lib.vbb_joint_embed_bwd_workspace(B, T, R, H)
    assert ws_n >= 4 * H
    ins = [Guard.of(t) for t in (dy, x, mean, rstd, gt, gv)]
    dxt, dxv, ws = Guard(B * T * H), Guard(B * R * H), Guard.filled(ws_n, NAN)
    sums = [Guard.filled(H, NAN) for _ in range(4)]
    rc = lib.vbb_joint_embed_bwd(_st(), B, T, R, H, *[i.ptr for i in ins], dxt.ptr, dxv.ptr, *[s.ptr for s in sums], ws.ptr)
    assert rc == 0, rc
    what = "vbb_joint_embed_bwd %s" % ((B, T, R, H),)
    ws.check(what + " workspace")
    return [dxt.cpu(what).view(B * T, H), dxv.cpu(what).view(B * R, H)] + [s.cpu(what) for s in sums]


@pytest.mark.parametrize("B,T,R,H", SHAPES)
def test_joint_embedding_backward_on_a_nan_workspace_is_right_and_bit_reproducible(B, T, R, H):
    S = T + R
    x, dy = _rand(B, S, H, seed=1, scale=2.0) + 0.3, _rand(B, S, H, seed=2)
    (gt, bt), (gv, bv) = _ln_params(H, 3), _ln_params(H, 4)
    segs = {"text": (slice(0, T), gt, bt), "image": (slice(T, S), gv, bv)}
    mean, rstd = torch.empty(B, S), torch.empty(B, S)
    refs = {}
    for name, (sl, g, b) in segs.items():
        xs, dys = x[:, sl].reshape(-1, H), dy[:, sl].reshape(-1, H)
        fwd = RB.ln64(xs, g, b, 1e-12)
        mean[:, sl], rstd[:, sl] = fwd["mean"].float().view(B, -1), fwd["rstd"].float().view(B, -1)
        refs[name] = RB.ln_backward64(xs, dys, g, 1e-12)
    got = _joint_bwd(B, T, R, H, dy, x, mean, rstd, gt, gv)
    for name, dx, dg, db in (("text", got[0], got[2], got[3]), ("image", got[1], got[4], got[5])):
        ref = refs[name]
        # dx: tests/test_backward_gpu.py::test_layernorm_backward's bar; column sums: fp32 accumulation (as vb_layernorm_bwd's)
        scale = max(1.0, float(ref["dx"].abs().max()))
        assert torch.isfinite(dx).all(), name
        assert float((dx.double() - ref["dx"]).abs().max()) <= 6e-5 * scale, name
        _within(dg, ref["dgamma"], 3e-6 * ref["dgamma_mag"] + 1e-6, name + " dgamma")
        _within(db, ref["dbeta"], 3e-6 * ref["dbeta_mag"] + 1e-6, name + " dbeta")
    again = _joint_bwd(B, T, R, H, dy, x, mean, rstd, gt, gv)
    for a, c in zip(got, again):
        assert torch.equal(_bits(a), _bits(c)), "two calls differ"


# ---------------------------------------------------------------------------------------------------------------------
# vbb_text_embed_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _text_bwd(fn, flags, ids, seg, dx, base):
    """One scatter launch into guarded COPIES of the tables `base` = (word, pos, type) -> the three tables on the CPU."""
    B, T = ids.shape
    H = dx.shape[-1]
    gi, gs, gd = Guard.of(ids), Guard.of(seg), Guard.of(dx)
    tabs = [Guard.of(t) for t in base]
    rc = fn(_st(), B, T, H, base[0].shape[0], base[2].shape[0], 0, gi.ptr, gs.ptr, None, gd.ptr, tabs[0].ptr, tabs[1].ptr,
            tabs[2].ptr, None, *flags)
    assert rc == 0, rc
    return [t.cpu("text_embed_bwd").view(b.shape) for t, b in zip(tabs, base)]


def _scatter64(ids, seg, dx, base, skip):
    """float64 tables after the scatter and the sums of |terms| added to each row."""
    B, T = ids.shape
    H = dx.shape[-1]
    d = dx.double().reshape(-1, H)
    out, mag = [b.double().clone() for b in base], [torch.zeros_like(b, dtype=torch.float64) for b in base]
    pos_idx = torch.arange(T).repeat(B)
    for tab, idx, skip0 in ((0, ids.reshape(-1), True), (1, pos_idx, skip), (2, seg.reshape(-1), skip)):
        ok = (idx >= 0) & (idx < base[tab].shape[0]) & ((idx != 0) if skip0 else torch.ones_like(idx, dtype=torch.bool))
        out[tab].index_add_(0, idx[ok], d[ok])
        mag[tab].index_add_(0, idx[ok], d[ok].abs())
    return out, mag


@pytest.mark.parametrize("B,T,H", [(3, 7, 64), (25, 7, 768), (2, 38, 768)])
def test_text_embed_bwd_with_padding_rows_is_the_plain_scatter_except_rows_zero(B, T, H):
    N = _N()
    N.ensure_deterministic(torch.device(DEV))
    assert N.deterministic_enabled()
    lib = _lib()
    gen = torch.Generator().manual_seed(B + H)
    ids, seg = torch.randint(0, VOCAB, (B, T), generator=gen), torch.randint(0, N_TYPES, (B, T), generator=gen)
    dx = _rand(B, T, H, seed=5)
    # the tables hold an earlier micro-batch's gradient: a skipped row must keep it, bit for bit
    base = (_rand(VOCAB, H, seed=6), _rand(T, H, seed=7), _rand(N_TYPES, H, seed=8))
    plain = _text_bwd(lib.vb_text_embed_bwd, (), ids, seg, dx, base)
    off = _text_bwd(lib.vbb_text_embed_bwd, (0, 0), ids, seg, dx, base)
    for a, c in zip(plain, off):
        assert torch.equal(_bits(a), _bits(c)), "flags off: not vb_text_embed_bwd"
    on = _text_bwd(lib.vbb_text_embed_bwd, (1, 1), ids, seg, dx, base)
    assert torch.equal(_bits(on[0]), _bits(plain[0]))
    for tab in (1, 2):
        assert torch.equal(_bits(on[tab][0]), _bits(base[tab][0])), "row 0 was touched"
        assert torch.equal(_bits(on[tab][1:]), _bits(plain[tab][1:]))
        assert not torch.equal(plain[tab][0], base[tab][0])
    only_pos = _text_bwd(lib.vbb_text_embed_bwd, (1, 0), ids, seg, dx, base)
    assert torch.equal(_bits(only_pos[1]), _bits(on[1])) and torch.equal(_bits(only_pos[2]), _bits(plain[2]))
    # the counted atomics fallback (deterministic setting off): same rows untouched, the rest right
    assert N.set_deterministic(False) is True
    try:
        atom = _text_bwd(lib.vbb_text_embed_bwd, (1, 1), ids, seg, dx, base)
    finally:
        N.set_deterministic(True)
    want, mag = _scatter64(ids, seg, dx, base, skip=True)
    for tab in range(3):
        if tab:
            assert torch.equal(_bits(atom[tab][0]), _bits(base[tab][0])), "atomics: row 0 was touched"
        _within(atom[tab], want[tab], 3e-6 * mag[tab] + 1e-6, "atomics table %d" % tab)
        _within(on[tab], want[tab], 3e-6 * mag[tab] + 1e-6, "ordered table %d" % tab)


# ---------------------------------------------------------------------------------------------------------------------
# vbb_tanh_fwd / vbb_tanh_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _tanh_sweep():
    x = torch.linspace(-12.0, 12.0, 4096, dtype=torch.float64).float()
    extra = torch.tensor([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 20.0, -20.0, float("inf"), float("-inf"), NAN], dtype=torch.float32)
    return torch.cat([x, extra])


def test_tanh_forward_and_backward_over_a_sweep_with_the_tails():
    x = _tanh_sweep()
    n = x.numel()
    xd, y = Guard.of(x), Guard(n)
    assert _lib().vbb_tanh_fwd(_st(), n, xd.ptr, y.ptr) == 0
    y = y.cpu("vbb_tanh_fwd")
    want = torch.tanh(x.double())
    fin = ~torch.isnan(x)
    assert torch.equal(torch.isnan(y), ~fin)
    err = (y.double() - want)[fin].abs()
    print("vbb_tanh_fwd: max |err| against float64 tanh over %d points = %.3e" % (int(fin.sum()), float(err.max())))
    assert float(y[fin].abs().max()) <= 1.0
    assert float(err.max()) <= 1e-6, "a wrong formula, not rounding"
    assert float(y[x == float("inf")]) == 1.0 and float(y[x == float("-inf")]) == -1.0
    assert float(y[x == 20.0]) == 1.0 and float(y[x == -20.0]) == -1.0
    assert bool((y[x == 0.0] == 0.0).all())
    # backward from the forward's own fp32 output: dx = dy * (1 - y * y), three fp32 roundings
    dy = _rand(n, seed=3)
    yd, dyd, dx = Guard.of(y), Guard.of(dy), Guard(n)
    assert _lib().vbb_tanh_bwd(_st(), n, dyd.ptr, yd.ptr, dx.ptr) == 0
    dx = dx.cpu("vbb_tanh_bwd")
    want_dx = dy.double() * (1.0 - y.double() * y.double())
    assert torch.equal(torch.isnan(dx), ~fin)
    berr = (dx.double() - want_dx)[fin].abs()
    assert bool((berr <= 4 * U * dy.double().abs()[fin] + 1e-37).all()), float(berr.max())
    assert bool((dx[y.abs() == 1.0] == 0.0).all())
    # in place, and a length that is no multiple of the block
    m = 1031
    buf = Guard.of(x[:m])
    assert _lib().vbb_tanh_fwd(_st(), m, buf.ptr, buf.ptr) == 0
    assert torch.equal(_bits(buf.cpu("in place")), _bits(y[:m]))
