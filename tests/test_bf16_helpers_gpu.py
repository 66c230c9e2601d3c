"""The helper kernels of the bf16 training stream, called directly (csrc/bf16_helpers.hip, layernorm.hip): the
casts that carry every value across the fp32 / bf16 border, the weight shadows, the bf16 column sum and the bf16 LayerNorm
at the edges of its shape range. The stream's own tests (test_bf16_stream_gpu.py) reach them only at the model's widths.

Rules of this file:
  * the C entry points are called through vilbert._native.lib() with raw pointers (strides, offsets, optional outputs);
  * references are float64 on the CPU from the same bf16 values; a pure conversion is compared with torch's CPU cast, bit
    for bit;
  * every output buffer lies between two canary margins (bytes 0x5A) which are checked afterwards; where a kernel writes a
    rectangle inside a larger buffer, the WHOLE buffer is compared with an image built on the CPU (canary outside);
  * tolerances: helpers.close16 - fp32 accumulation 3e-6 sum|terms| + 1e-5, plus one bf16 rounding (|want| / 256) for a
    bf16 output. The attention case adds the rounding of the probabilities to bf16 (see there).

Rounding contract (csrc/bf16_round.h; tests/test_bf16_round.py holds the header itself to it on the CPU): a non-NaN fp32
value is stored as torch's CPU cast, a NaN as a bf16 NaN - over every rounding decision (helpers.rounding_patterns).
"""
import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
E_BADARG, E_ALIGN, E_RANGE = -1, -2, -3
CANARY, CANARY16 = 0x5A, 0x5A5A
NAN16, INF16 = 0xffff, 0x7f80      # the all-ones NaN the add-and-shift rounding stored as +0


def _lib():
    from vilbert import _native
    return _native.lib()


def _st():
    from vilbert import _native
    return _native.stream_ptr()


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Guard:
    """n elements of `dtype` on the device between two canary margins; the payload starts as canary bytes too."""
    MARGIN = 512

    def __init__(self, n, dtype):
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * self.MARGIN + self.nbytes,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.buf[self.MARGIN:self.MARGIN + self.nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        torch.cuda.synchronize()
        m = self.MARGIN
        assert bool((self.buf[:m] == CANARY).all()) and bool((self.buf[m + self.nbytes:] == CANARY).all()), \
            "%s: wrote outside its buffer" % what

    def untouched(self, what):
        self.check(what)
        assert bool((self.buf == CANARY).all()), "%s: wrote although it returned an error" % what

    def u16(self, what):
        self.check(what)
        return self.t.view(torch.int16).cpu().numpy().view(np.uint16)

    def u32(self, what):
        self.check(what)
        return self.t.view(torch.int32).cpu().numpy().view(np.uint32)


def _f32_from_bits(bits32):
    """CPU fp32 tensor with exactly these bits (uint32 array)."""
    return torch.from_numpy(np.ascontiguousarray(bits32).view(np.int32).copy()).view(torch.float32)


def _bf16_from_bits(bits16):
    return torch.from_numpy(np.ascontiguousarray(bits16).view(np.int16).copy()).view(BF16)


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# rounding contract, exhaustive over the rounding decision
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def patterns():
    bits = helpers.rounding_patterns()                  # 524,288 = 8 x 64 x 64 x 16
    bits.setflags(write=False)
    return bits, _f32_from_bits(bits).to(DEV)


def test_rounding_contract_cast(patterns):
    bits, x = patterns
    out = Guard(bits.size, torch.int16)
    assert _lib().vb_cast_f32_bf16(_st(), bits.size, x.data_ptr(), out.ptr) == 0
    helpers.check_rounding_contract(bits, out.u16("vb_cast_f32_bf16"), "vb_cast_f32_bf16")


def test_rounding_contract_cast_rows(patterns):
    bits, x = patterns
    rows, n, ldx, ldy = 2048, 256, 260, 264
    src = torch.full((rows, ldx), float("nan"), device=DEV)
    src[:, :n] = x.view(rows, n)
    out = Guard(rows * ldy, torch.int16)
    assert _lib().vb_cast_rows_f32_bf16(_st(), rows, n, src.data_ptr(), ldx, out.ptr, ldy) == 0
    got = out.u16("vb_cast_rows_f32_bf16").reshape(rows, ldy)
    helpers.check_rounding_contract(bits, np.ascontiguousarray(got[:, :n]), "vb_cast_rows_f32_bf16")
    assert (got[:, n:] == 0).all()


@pytest.mark.parametrize("entry", ["single", "multi"])
def test_rounding_contract_weight_shadows(patterns, entry):
    bits, x = patterns
    rows, cols = 512, 1024
    w = x.view(rows, cols)
    w16, wt16 = Guard(rows * cols, torch.int16), Guard(rows * cols, torch.int16)
    if entry == "single":
        assert _lib().vb_weight_shadow_bf16(_st(), rows, cols, w.data_ptr(), cols, w16.ptr, cols, wt16.ptr, rows) == 0
    else:                                               # two stacked segments of 256 rows, as ops16._refresh_all lays them out
        seg = rows // 2
        tab = _shadow_table([(w.data_ptr() + 4 * s * seg * cols, w16.ptr + 2 * s * seg * cols, wt16.ptr + 2 * s * seg,
                              seg, cols, cols, rows) for s in range(2)])
        assert _lib().vb_weight_shadow_multi(_st(), 2, tab["dev"].data_ptr(), tab["tiles"]) == 0
    b2 = bits.reshape(rows, cols)
    helpers.check_rounding_contract(b2, w16.u16("w16").reshape(rows, cols), "w16 (%s)" % entry)
    helpers.check_rounding_contract(np.ascontiguousarray(b2.T), wt16.u16("wt16").reshape(cols, rows), "wt16 (%s)" % entry)


def test_cast_bf16_f32_is_exact_and_the_round_trip_idempotent(patterns):
    from vilbert import ops16
    all16 = np.arange(1 << 16, dtype=np.uint16)
    out, src = Guard(all16.size, torch.int32), _bf16_from_bits(all16).to(DEV)
    assert _lib().vb_cast_bf16_f32(_st(), all16.size, src.data_ptr(), out.ptr) == 0
    assert (out.u32("vb_cast_bf16_f32") == all16.astype(np.uint32) << 16).all()
    # the wrappers: bf16 -> fp32 -> bf16 gives the same bits for every non-NaN pattern, NaNs stay NaN; and
    # cast_f32(cast_bf16(x)) is a fixed point of the pair for every fp32 rounding pattern
    back = _bits16(ops16.cast_bf16(ops16.cast_f32(src)))
    nan16 = (all16 & 0x7fff) > 0x7f80
    assert (back[~nan16] == all16[~nan16]).all() and ((back[nan16] & 0x7fff) > 0x7f80).all()
    _bits, x = patterns
    once = ops16.cast_f32(ops16.cast_bf16(x))
    twice = ops16.cast_f32(ops16.cast_bf16(once))
    assert torch.equal(once.view(torch.int32), twice.view(torch.int32))
    # a non-contiguous input goes through the wrapper's copy
    xt = x.view(512, 1024).t()
    assert torch.equal(ops16.cast_bf16(xt).view(torch.int16), ops16.cast_bf16(xt.contiguous()).view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------------
# casts: shapes and error returns
# ---------------------------------------------------------------------------------------------------------------------
def _special_f32(n, seed):
    """n fp32 values: normal draws over many magnitudes with ties, subnormals, infinities and zeros mixed in (no NaN)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-140, 127, (n,), generator=g).float())
    bits = x.view(torch.int32).numpy().view(np.uint32).copy()
    bits[::5] = (bits[::5] & 0xffff0000) | 0x8000                       # exact ties
    bits[3::11] &= 0x807fffff                                           # fp32 subnormals / zeros
    bits[7::13] = 0x7f800000
    bits[8::17] = 0xff7fffff                                            # rounds to -Inf
    return bits


@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16, 2047, 2048, 2049, 2056, 65537])
def test_cast_shapes(n):
    # 8 values per thread, 256 threads per block; the thread after the last full one takes the tail: n < 8 is a tail-only
    # launch, n % 8 == 0 has none, and at n = 2048 .. 2056 the tail thread is the first thread of a second block
    bits = _special_f32(n, n)
    out, src = Guard(n, torch.int16), _f32_from_bits(bits).to(DEV)
    assert _lib().vb_cast_f32_bf16(_st(), n, src.data_ptr(), out.ptr) == 0
    got = out.u16("vb_cast_f32_bf16")
    assert (got == helpers.torch_cast_bits(bits)).all()
    b16 = np.random.default_rng(n).integers(0, 1 << 16, n).astype(np.uint16)
    out32, src16 = Guard(n, torch.int32), _bf16_from_bits(b16).to(DEV)
    assert _lib().vb_cast_bf16_f32(_st(), n, src16.data_ptr(), out32.ptr) == 0
    assert (out32.u32("vb_cast_bf16_f32") == b16.astype(np.uint32) << 16).all()


@pytest.mark.parametrize("rows,n,ldx,ldy", [(1, 1, 4, 8), (3, 5, 8, 8), (4, 8, 8, 8), (5, 12, 12, 256), (7, 250, 252, 256),
                                            (2, 257, 260, 512), (3, 30522, 30524, 30720)])
def test_cast_rows_shapes(rows, n, ldx, ldy):
    bits = _special_f32(rows * n, rows * 1000 + n).reshape(rows, n)
    src = torch.full((rows, ldx), float("nan"))
    src[:, :n] = _f32_from_bits(bits).view(rows, n)
    out, srcd = Guard(rows * ldy, torch.int16), src.to(DEV)
    assert _lib().vb_cast_rows_f32_bf16(_st(), rows, n, srcd.data_ptr(), ldx, out.ptr, ldy) == 0
    got = out.u16("vb_cast_rows_f32_bf16").reshape(rows, ldy)
    assert (got[:, :n] == helpers.torch_cast_bits(bits.reshape(-1)).reshape(rows, n)).all()
    assert (got[:, n:] == 0).all(), "the padding columns must be +0"


def test_cast_error_returns():
    lib, x = _lib(), torch.zeros(4096, device=DEV)
    x16 = torch.zeros(4096, dtype=BF16, device=DEV)
    out = Guard(4096, torch.int16)
    out32 = Guard(4096, torch.int32)
    assert lib.vb_cast_f32_bf16(_st(), 64, x.data_ptr() + 4, out.ptr) == E_ALIGN
    assert lib.vb_cast_f32_bf16(_st(), 64, x.data_ptr(), out.ptr + 2) == E_ALIGN
    assert lib.vb_cast_f32_bf16(_st(), 0, x.data_ptr(), out.ptr) == E_BADARG
    assert lib.vb_cast_bf16_f32(_st(), 64, x16.data_ptr() + 2, out32.ptr) == E_ALIGN
    assert lib.vb_cast_bf16_f32(_st(), 64, x16.data_ptr(), out32.ptr + 4) == E_ALIGN
    rows = lib.vb_cast_rows_f32_bf16
    assert rows(_st(), 2, 8, x.data_ptr() + 4, 8, out.ptr, 8) == E_ALIGN
    assert rows(_st(), 2, 8, x.data_ptr(), 8, out.ptr + 8, 8) == E_ALIGN
    assert rows(_st(), 2, 4, x.data_ptr(), 8, out.ptr, 12) == E_ALIGN          # ldy % 8
    assert rows(_st(), 2, 4, x.data_ptr(), 6, out.ptr, 8) == E_ALIGN           # ldx % 4
    assert rows(_st(), 2, 8, x.data_ptr(), 4, out.ptr, 8) == E_BADARG          # ldx < n
    assert rows(_st(), 2, 0, x.data_ptr(), 8, out.ptr, 8) == E_BADARG
    assert rows(_st(), 2, -4, x.data_ptr(), 8, out.ptr, 8) == E_BADARG
    out.untouched("cast error returns")
    out32.untouched("cast error returns")


# ---------------------------------------------------------------------------------------------------------------------
# weight shadows
# ---------------------------------------------------------------------------------------------------------------------
SHADOW_REC = np.dtype([("w", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("ld16", "<i8"),
                       ("ldt", "<i8"), ("tile0", "<i8")])          # vb_shadow_seg, as ops16._refresh_all builds it


def _shadow_table(segs):
    """segs: (w, w16, wt16, rows, cols, ld16, ldt) per segment -> the device table and its tile count."""
    rows, tile0 = [], 0
    for s in segs:
        rows.append(tuple(s) + (tile0,))
        tile0 += (s[3] // 64) * (s[4] // 64)
    host = np.array(rows, dtype=SHADOW_REC)
    assert SHADOW_REC.itemsize == 56                   # sizeof(vb_shadow_seg)
    return {"dev": torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(DEV), "tiles": tile0}


@pytest.mark.parametrize("which", ["w16", "wt16", "both"])
@pytest.mark.parametrize("rows,cols", [(64, 64), (64, 192), (192, 64), (128, 320)])
def test_weight_shadow_strides_offsets_and_optional_outputs(rows, cols, which):
    """Every leading dimension larger than the matrix, wt16 offset by a column count inside a wider transposed buffer (the
    second segment of a stacked weight), one or both outputs: the whole buffers against images built on the CPU."""
    ldw, ld16, col_off = cols + 4, cols + 8, 64
    ldt = col_off + rows + 12
    src = torch.full((rows, ldw), float("nan"))
    src[:, :cols] = _rand(rows, cols, seed=rows + cols)
    want = src[:, :cols].to(BF16).view(torch.int16)
    g16, gt16, srcd = Guard(rows * ld16, torch.int16), Guard(cols * ldt, torch.int16), src.to(DEV)
    rc = _lib().vb_weight_shadow_bf16(_st(), rows, cols, srcd.data_ptr(), ldw, g16.ptr if which != "wt16" else None, ld16,
                                      gt16.ptr + 2 * col_off if which != "w16" else None, ldt)
    assert rc == 0
    img16 = torch.full((rows, ld16), CANARY16, dtype=torch.int16)
    imgt = torch.full((cols, ldt), CANARY16, dtype=torch.int16)
    if which != "wt16":
        img16[:, :cols] = want
    if which != "w16":
        imgt[:, col_off:col_off + rows] = want.t()
    g16.check("w16")
    gt16.check("wt16")
    assert torch.equal(g16.t.cpu().view(rows, ld16), img16), "w16"
    assert torch.equal(gt16.t.cpu().view(cols, ldt), imgt), "wt16"


def test_weight_shadow_error_returns():
    f = _lib().vb_weight_shadow_bf16
    w = torch.zeros(128 * 128, device=DEV)
    a, b = Guard(128 * 128, torch.int16), Guard(128 * 128, torch.int16)
    assert f(_st(), 96, 64, w.data_ptr(), 64, a.ptr, 64, b.ptr, 96) == E_ALIGN          # rows % 64
    assert f(_st(), 64, 96, w.data_ptr(), 96, a.ptr, 96, b.ptr, 64) == E_ALIGN          # cols % 64
    assert f(_st(), 64, 128, w.data_ptr(), 128, a.ptr, 64, b.ptr, 64) == E_ALIGN        # ld16 < cols
    assert f(_st(), 128, 64, w.data_ptr(), 64, a.ptr, 64, b.ptr, 64) == E_ALIGN         # ldt < rows
    assert f(_st(), 64, 64, w.data_ptr(), 64, None, 64, None, 64) == E_BADARG           # nothing to write
    assert f(_st(), 64, 64, None, 64, a.ptr, 64, b.ptr, 64) == E_BADARG
    a.untouched("shadow error returns")
    b.untouched("shadow error returns")


# 7 segments, 1 + 1 + 6 + 10 + 3 + 4 + 1 = 26 tiles: two single-tile segments side by side (tile0 = 0, 1), every segment's
# first and last tile on a boundary of the bisection
SHADOW_SEGS = [(64, 64), (64, 64), (192, 128), (128, 320), (64, 192), (256, 64), (64, 64)]


@pytest.mark.parametrize("n_segs", [1, 2, len(SHADOW_SEGS)])
def test_weight_shadow_multi_table(n_segs):
    shapes = SHADOW_SEGS[:n_segs]
    gap = 72                                           # canary elements between two segments' outputs
    ws, lay, off16, offt = [], [], gap, gap
    for i, (r, c) in enumerate(shapes):
        ld16, ldt = c + 4 * (i % 3), r + 8 * (i % 2)
        lay.append((off16, ld16, offt, ldt))
        off16 += r * ld16 + gap
        offt += c * ldt + gap
        ws.append(_rand(r, c, seed=50 + i))
    g16, gt = Guard(off16, torch.int16), Guard(offt, torch.int16)
    wd = [w.to(DEV) for w in ws]
    tab = _shadow_table([(wd[i].data_ptr(), g16.ptr + 2 * lay[i][0], gt.ptr + 2 * lay[i][2], r, c, lay[i][1], lay[i][3])
                         for i, (r, c) in enumerate(shapes)])
    assert tab["tiles"] == sum((r // 64) * (c // 64) for r, c in shapes)
    assert _lib().vb_weight_shadow_multi(_st(), n_segs, tab["dev"].data_ptr(), tab["tiles"]) == 0
    img16 = torch.full((off16,), CANARY16, dtype=torch.int16)
    imgt = torch.full((offt,), CANARY16, dtype=torch.int16)
    for i, (r, c) in enumerate(shapes):
        o16, ld16, ot, ldt = lay[i]
        want = ws[i].to(BF16).view(torch.int16)
        img16[o16:o16 + r * ld16].view(r, ld16)[:, :c] = want
        imgt[ot:ot + c * ldt].view(c, ldt)[:, :r] = want.t()
    g16.check("w16 of the table")
    gt.check("wt16 of the table")
    assert torch.equal(g16.t.cpu(), img16), "w16: a segment differs from its reference or a gap was written"
    assert torch.equal(gt.t.cpu(), imgt), "wt16: a segment differs from its reference or a gap was written"
    assert _lib().vb_weight_shadow_multi(_st(), 0, tab["dev"].data_ptr(), tab["tiles"]) == E_BADARG
    assert _lib().vb_weight_shadow_multi(_st(), n_segs, None, tab["tiles"]) == E_BADARG
    assert _lib().vb_weight_shadow_multi(_st(), n_segs, tab["dev"].data_ptr(), 0) == E_BADARG


# ---------------------------------------------------------------------------------------------------------------------
# vb_colsum_bf16
# ---------------------------------------------------------------------------------------------------------------------
COLSUM_SHAPES = [(1, 4), (3, 252), (63, 256), (64, 260), (65, 1024), (257, 4), (4100, 252), (1, 1024), (64, 256), (65, 260),
                 (4100, 1024), (257, 256)]      # every row count around the 64 row slabs x every width around the 256-column block


@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("rows,cols", COLSUM_SHAPES)
def test_colsum_bf16(rows, cols, pad):
    lib = _lib()
    ldx = cols + pad
    xb = torch.full((rows, ldx), float("nan"), dtype=BF16)
    xb[:, :cols] = _rand(rows, cols, seed=rows + cols).to(BF16)
    x = xb[:, :cols]
    out0 = _rand(cols, seed=7)
    ws_floats = lib.vb_colsum_bf16_workspace(cols)
    assert ws_floats >= cols
    xd = xb.to(DEV)
    outs = []
    for _ in range(2):
        out, ws = Guard(cols, torch.float32), Guard(ws_floats, torch.float32)
        out.t.copy_(out0)
        assert lib.vb_colsum_bf16(_st(), rows, cols, xd.data_ptr(), ldx, out.ptr, ws.ptr) == 0
        out.check("colsum out")
        ws.check("colsum workspace")
        outs.append(out.t.clone())
    helpers.close16(outs[0], x.double().sum(0) + out0.double(), x.double().abs().sum(0), "column sums, added into out")
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), "two runs differ"


def test_colsum_error_returns():
    lib = _lib()
    x = torch.zeros(64 * 64, dtype=BF16, device=DEV)
    out, ws = Guard(64, torch.float32), Guard(64 * 64, torch.float32)
    assert lib.vb_colsum_bf16(_st(), 8, 6, x.data_ptr(), 8, out.ptr, ws.ptr) == E_ALIGN              # cols % 4
    assert lib.vb_colsum_bf16(_st(), 8, 16, x.data_ptr(), 12, out.ptr, ws.ptr) == E_ALIGN             # ldx < cols
    assert lib.vb_colsum_bf16(_st(), 8, 16, x.data_ptr(), 16, out.ptr, ws.ptr + 4) == E_ALIGN        # workspace
    assert lib.vb_colsum_bf16(_st(), 8, 16, x.data_ptr() + 2, 16, out.ptr, ws.ptr) == E_ALIGN
    assert lib.vb_colsum_bf16(_st(), 0, 16, x.data_ptr(), 16, out.ptr, ws.ptr) == E_BADARG
    assert lib.vb_colsum_bf16(_st(), 8, 16, x.data_ptr(), 16, out.ptr, None) == E_BADARG
    out.untouched("colsum error returns")
    ws.untouched("colsum error returns")


# ---------------------------------------------------------------------------------------------------------------------
# bf16 LayerNorm at the edges
# ---------------------------------------------------------------------------------------------------------------------
EPS = 1e-12


def _ln_fwd(x, g, b, stats=True):
    """vb_layernorm_fwd_bf16 on guarded outputs: (y Guard, mean Guard or None, rstd Guard or None)."""
    rows, cols = x.shape
    y = Guard(rows * cols, BF16)
    mean = Guard(rows, torch.float32) if stats else None
    rstd = Guard(rows, torch.float32) if stats else None
    rc = _lib().vb_layernorm_fwd_bf16(_st(), rows, cols, x.data_ptr(), g.data_ptr(), b.data_ptr(), EPS, y.ptr,
                                      mean.ptr if stats else None, rstd.ptr if stats else None)
    assert rc == 0
    for gd in (y, mean, rstd):
        if gd is not None:
            gd.check("LayerNorm forward")
    return y, mean, rstd


def _ln_bwd(dy, x, mean, rstd, g):
    """vb_layernorm_bwd_bf16 on guarded outputs, dgamma / dbeta pre-filled with NaN: (dx, dgamma, dbeta) tensors."""
    rows, cols = x.shape
    lib = _lib()
    dx, dg, db = Guard(rows * cols, BF16), Guard(cols, torch.float32), Guard(cols, torch.float32)
    ws = Guard(lib.vb_layernorm_bwd_bf16_workspace(rows, cols), torch.float32)
    dg.t.fill_(float("nan"))
    db.t.fill_(float("nan"))
    rc = lib.vb_layernorm_bwd_bf16(_st(), rows, cols, dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g.data_ptr(),
                                   dx.ptr, dg.ptr, db.ptr, ws.ptr, None, 0.0, 0)
    assert rc == 0
    for gd in (dx, dg, db, ws):
        gd.check("LayerNorm backward")
    return dx.t.view(rows, cols), dg.t, db.t


def _ln_case(x, dy, g, b, what):
    rows, cols = x.shape
    ref = helpers.layernorm16_reference(x, dy, g, b, EPS)
    xd, dyd, gd, bd = x.to(DEV), dy.to(DEV), g.to(DEV), b.to(DEV)
    y, mean, rstd = _ln_fwd(xd, gd, bd)
    helpers.close16(y.t.view(rows, cols), ref["y"], torch.ones(rows, cols, dtype=torch.float64) * 4, what + ": forward")
    assert (mean.t.cpu().double() - ref["mean"]).abs().max() < 1e-5
    assert (rstd.t.cpu().double() * torch.sqrt(ref["var"] + EPS) - 1).abs().max() < 1e-5
    y2, _, _ = _ln_fwd(xd, gd, bd, stats=False)
    assert torch.equal(y2.t.view(torch.int16), y.t.view(torch.int16)), what + ": y depends on want_stats"
    dx, dgam, dbet = _ln_bwd(dyd, xd, mean.t, rstd.t, gd)
    scale = torch.ones(rows, cols, dtype=torch.float64) * float(ref["dx"].abs().max()) * 4
    helpers.close16(dx, ref["dx"], scale, what + ": dx")
    helpers.close16(dgam, ref["dgamma"], (dy.double() * ref["xh"]).abs().sum(0) + 1, what + ": dgamma (overwritten)")
    helpers.close16(dbet, ref["dbeta"], dy.double().abs().sum(0) + 1, what + ": dbeta (overwritten)")
    dx2, dgam2, dbet2 = _ln_bwd(dyd, xd, mean.t, rstd.t, gd)
    assert torch.equal(dx2.view(torch.int16), dx.view(torch.int16)) and torch.equal(dgam2, dgam) and torch.equal(dbet2, dbet), \
        what + ": two backward runs differ"


def _ln_inputs(rows, cols):
    x = (_rand(rows, cols, seed=rows + cols) * 2 + 0.3).to(BF16)
    dy = _rand(rows, cols, seed=rows + cols + 1).to(BF16)
    return x, dy, 1 + 0.1 * _rand(cols, seed=3), 0.1 * _rand(cols, seed=4)


# a lane holds 4 columns of every 256-column chunk, one instantiation per chunk count: a partly filled last chunk for each
@pytest.mark.parametrize("cols", [4, 8, 252, 260, 508, 516, 772, 1020])
def test_layernorm16_partly_filled_chunks(cols):
    _ln_case(*_ln_inputs(37, cols), "37 x %d" % cols)


# forward: 1 row per wave below 4,096 rows, 2 up to 16,384, then 4; (16 | 17) x 1024: the backward's 16 rows per block
@pytest.mark.parametrize("rows,cols", [(1, 64), (2, 64), (4095, 64), (4096, 64), (4097, 64), (16383, 64), (16384, 64), (16385, 64),
                                       (16, 1024), (17, 1024)])
def test_layernorm16_row_thresholds(rows, cols):
    _ln_case(*_ln_inputs(rows, cols), "%d x %d" % (rows, cols))


@pytest.mark.parametrize("cols", [252, 1024])
def test_layernorm16_constant_rows_give_beta(cols):
    x, _dy, g, b = _ln_inputs(9, cols)
    consts = torch.tensor([0.30078125, -1.5, 0.0, 300.0], dtype=BF16)         # exact in bf16; every partial sum exact in fp32
    x[1:5] = consts[:, None]
    y, _, rstd = _ln_fwd(x.to(DEV), g.to(DEV), b.to(DEV))
    yb = y.t.view(9, cols).cpu()
    assert torch.isfinite(yb.float()).all() and torch.isfinite(rstd.t).all()
    for r in range(1, 5):       # variance 0: y = gamma * 0 * rstd + beta
        assert torch.equal(yb[r].view(torch.int16), b.to(BF16).view(torch.int16)), "row %d" % r
    helpers.close16(yb, helpers.layernorm16_reference(x, x, g, b, EPS)["y"], torch.ones(9, cols, dtype=torch.float64) * 4, "the other rows")


def test_layernorm16_large_mean_small_deviation():
    """Rows with mean 300 and standard deviation 0.5 (bf16 spacing at 300 is 2: 1 / 32 of the values at 298, 1 / 32 at 302,
    the rest at 300). E[x^2] - mean^2 in fp32 is 90000.25 - 90000 with an ulp of 0.0078: 3 % of the variance - a one-pass
    variance misses the bar by a factor of four."""
    rows, cols = 6, 1024
    base = torch.full((cols,), 300.0)
    base[:32], base[32:64] = 298.0, 302.0
    x = torch.stack([base[torch.randperm(cols, generator=torch.Generator().manual_seed(r))] for r in range(rows)]).to(BF16)
    assert float(x.double().mean()) == 300.0 and abs(float(x.double().std(unbiased=False)) - 0.5) < 1e-12
    _x, dy, g, b = _ln_inputs(rows, cols)
    _ln_case(x, dy, g, b, "mean 300, deviation 0.5")


def test_layernorm16_workspace_and_error_returns():
    lib = _lib()
    for rows in (1, 15, 16, 17, 4101):
        for cols in (64, 1020):
            assert lib.vb_layernorm_bwd_bf16_workspace(rows, cols) == (rows + 15) // 16 * 2 * cols     # ops16.layernorm_bwd's buffer
    x = torch.zeros(8 * 1028 + 8, dtype=BF16, device=DEV)
    g = torch.ones(1028, device=DEV)
    stat = torch.ones(8, device=DEV)
    y, dx, dxd = Guard(8 * 1028, BF16), Guard(8 * 1028, BF16), Guard(8 * 1028, BF16)
    dg, db, ws = Guard(1028, torch.float32), Guard(1028, torch.float32), Guard(2 * 1028, torch.float32)

    def fwd(cols, xp=x.data_ptr(), yp=y.ptr):
        return lib.vb_layernorm_fwd_bf16(_st(), 8, cols, xp, g.data_ptr(), g.data_ptr(), EPS, yp, None, None)

    def bwd(cols, xp=x.data_ptr(), dyp=x.data_ptr(), dxdp=None, p=0.0):
        return lib.vb_layernorm_bwd_bf16(_st(), 8, cols, dyp, xp, stat.data_ptr(), stat.data_ptr(), g.data_ptr(), dx.ptr, dg.ptr,
                                         db.ptr, ws.ptr, dxdp, p, 1)
    for f in (fwd, bwd):
        assert f(1028) == E_RANGE and f(6) == E_RANGE and f(0) == E_RANGE
        assert f(64, xp=x.data_ptr() + 4) == E_ALIGN and f(64, xp=x.data_ptr() + 2) == E_ALIGN      # (8 bytes are required)
    assert fwd(64, yp=y.ptr + 4) == E_ALIGN
    assert bwd(64, dyp=x.data_ptr() + 4) == E_ALIGN
    assert bwd(64, dxdp=dxd.ptr, p=0.0) == E_BADARG and bwd(64, dxdp=dxd.ptr, p=1.0) == E_BADARG
    assert bwd(64, dxdp=dxd.ptr + 4, p=0.5) == E_ALIGN
    dxd.untouched("LayerNorm error returns")


# ---------------------------------------------------------------------------------------------------------------------
# non-finite values are never laundered
# ---------------------------------------------------------------------------------------------------------------------
def _poisoned(t, row, col, kind):
    """bf16 CPU tensor t with element (row, col) replaced by the all-ones NaN / +Inf."""
    t = t.clone()
    t.view(torch.int16)[row, col] = np.array([NAN16 if kind == "nan" else INF16], dtype=np.uint16).view(np.int16)[0]
    return t


def _close16_where_finite(got, want64, mag64, what, min_bad, extra64=None):
    """helpers.close16 on the elements whose float64 reference is finite; every other element (reference NaN or +-Inf) must
    be non-finite in `got`. At least `min_bad` reference elements must be non-finite (the case is not vacuous)."""
    g = got.detach().cpu().double()
    assert g.shape == want64.shape, what
    bad = ~torch.isfinite(want64)
    assert int(bad.sum()) >= min_bad, "%s: the reference has %d non-finite elements, expected >= %d" % (what, int(bad.sum()), min_bad)
    lost = bad & torch.isfinite(g)
    assert not lost.any(), "%s: %d of %d non-finite reference elements came out finite (first value %r)" % (
        what, int(lost.sum()), int(bad.sum()), float(g[lost][0]))
    ok = ~bad
    w = torch.where(ok, want64, torch.zeros_like(want64))
    m = torch.where(ok, mag64.expand_as(want64) if isinstance(mag64, torch.Tensor) else torch.full_like(want64, mag64),
                    torch.zeros_like(want64))
    gg = torch.where(ok, g, torch.zeros_like(g))
    extra = 0.0 if extra64 is None else torch.where(ok, extra64, torch.zeros_like(want64))
    helpers.close16(gg.to(got.dtype) if got.dtype == BF16 else gg.float(), w, m, what, extra64=extra)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_layernorm(kind):
    from vilbert import ops16
    rows, cols, pr, pc = 7, 8, 3, 5
    x, dy, g, b = _ln_inputs(rows, cols)
    one = torch.ones(rows, cols, dtype=torch.float64)
    xp = _poisoned(x, pr, pc, kind)
    ref = helpers.layernorm16_reference(xp, dy, g, b, EPS)
    assert not torch.isfinite(ref["y"][pr]).any() and torch.isfinite(ref["y"][torch.arange(rows) != pr]).all()
    y, mean, rstd = ops16.layernorm_fwd(xp.to(DEV), g.to(DEV), b.to(DEV), EPS, want_stats=True)
    _close16_where_finite(y, ref["y"], one * 4, "forward, poisoned x", cols)
    if kind == "nan":       # an fp32 operand carries the whole 32-bit payload into the store: beta[pc] = 0xffffffff
        bp = b.clone()
        bp.view(torch.int32)[pc] = -1
        yb, _, _ = ops16.layernorm_fwd(x.to(DEV), g.to(DEV), bp.to(DEV), EPS)
        _close16_where_finite(yb, helpers.layernorm16_reference(x, dy, g, bp, EPS)["y"], one * 4, "forward, poisoned beta", rows)
        assert not torch.isfinite(yb[:, pc].float()).any()
    clean = helpers.layernorm16_reference(x, dy, g, b, EPS)
    scale = one * float(clean["dx"].abs().max()) * 4
    # backward on the poisoned x (its row's statistics are non-finite): dx row, and dgamma in EVERY column
    dx, dgam, dbet = ops16.layernorm_bwd(dy.to(DEV), xp.to(DEV), mean, rstd, g.to(DEV))
    _close16_where_finite(dx, ref["dx"], scale, "dx, poisoned x", cols)
    assert not torch.isfinite(dgam).any(), "dgamma must be non-finite in every column"
    helpers.close16(dbet, ref["dbeta"], dy.double().abs().sum(0) + 1, "dbeta, poisoned x (sums dy only)")
    # backward with a gradient row that is non-finite in every column (what the layer above hands down once a row is lost)
    _y, mean, rstd = ops16.layernorm_fwd(x.to(DEV), g.to(DEV), b.to(DEV), EPS, want_stats=True)
    dyp = dy.clone()
    for c in range(cols):
        dyp = _poisoned(dyp, pr, c, kind)
    refp = helpers.layernorm16_reference(x, dyp, g, b, EPS)
    dx, dgam, dbet = ops16.layernorm_bwd(dyp.to(DEV), x.to(DEV), mean, rstd, g.to(DEV))
    _close16_where_finite(dx, refp["dx"], scale, "dx, poisoned dy row", cols)
    assert not torch.isfinite(dgam).any() and not torch.isfinite(dbet).any(), "dgamma / dbeta must be non-finite in every column"
    # one poisoned gradient element: its dx row, and its column of dgamma / dbeta
    dy1 = _poisoned(dy, pr, pc, kind)
    ref1 = helpers.layernorm16_reference(x, dy1, g, b, EPS)
    dx, dgam, dbet = ops16.layernorm_bwd(dy1.to(DEV), x.to(DEV), mean, rstd, g.to(DEV))
    _close16_where_finite(dx, ref1["dx"], scale, "dx, one poisoned dy", cols)
    _close16_where_finite(dgam, ref1["dgamma"], (dy.double() * clean["xh"]).abs().sum(0) + 1, "dgamma, one poisoned dy", 1)
    _close16_where_finite(dbet, ref1["dbeta"], dy.double().abs().sum(0) + 1, "dbeta, one poisoned dy", 1)


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_linear(kind):
    from vilbert import ops16
    M, n_out, K, pr = 5, 256, 128, 2
    x = _rand(M, K, seed=1).to(BF16)
    w = _rand(n_out, K, seed=2, scale=0.05)
    bias = _rand(n_out, seed=3)
    wd, bd = [w.to(DEV)], [bias.to(DEV)]
    w16 = w.to(BF16).double()
    xp = _poisoned(x, pr, 7, kind)
    pre = xp.double() @ w16.t() + bias.double()
    mag = x.double().abs() @ w16.abs().t() + 1.0
    y, _ = ops16.linear_fwd(xp.to(DEV), wd, bd)
    _close16_where_finite(y, pre, mag, "forward", n_out)
    y, d = ops16.linear_fwd(xp.to(DEV), wd, bd, "gelu", want_act_grad=True)
    _close16_where_finite(y, torch.nn.functional.gelu(pre), mag, "forward + GELU", n_out)
    assert not torch.isfinite(d[pr].float()).any() or kind == "inf", "GELU derivative of a NaN row"
    if kind == "nan":       # an fp32 operand carries the whole 32-bit payload into the epilogue: bias[9] = 0xffffffff
        bp = bias.clone()
        bp.view(torch.int32)[9] = -1
        clean_mag = x.double().abs() @ w16.abs().t() + 1.0
        pre_b = x.double() @ w16.t() + bp.double()
        y, _ = ops16.linear_fwd(x.to(DEV), wd, [bp.to(DEV)])
        _close16_where_finite(y, pre_b, clean_mag, "forward, poisoned bias", M)
        y, _ = ops16.linear_fwd(x.to(DEV), wd, [bp.to(DEV)], "gelu")
        _close16_where_finite(y, torch.nn.functional.gelu(pre_b), clean_mag, "forward + GELU, poisoned bias", M)
    dy = _rand(M, n_out, seed=4).to(BF16)
    dyp = _poisoned(dy, pr, 100, kind)
    want = dyp.double() @ w16
    _close16_where_finite(ops16.linear_bwd_input(dyp.to(DEV), wd, bd, K), want, dy.double().abs() @ w16.abs() + 1.0, "dgrad", K)
    ops16.shadow_cache_clear()


@pytest.mark.parametrize("kind", ["nan", "inf"])
def test_nonfinite_attention_value(kind):
    """A poisoned element of v reaches column c of every query row of its sample. Bound of the finite elements: the
    probabilities enter the second contraction rounded to bf16 (2^-9 each) next to a normaliser from the unrounded ones, the
    result is rounded once more: 2^-8 sum_j P |v| for the first two, close16's |want| / 256 for the store."""
    from vilbert import ops16
    B, heads, d, Sq, Sk = 2, 2, 32, 9, 7
    H = heads * d
    qkv_q = (_rand(B, Sq, 3 * H, seed=1) * 0.7).to(BF16)
    qkv_k = (_rand(B, Sk, 3 * H, seed=2) * 0.7).to(BF16)
    pb, pk, pc = 1, 3, 2 * H + 40                       # sample 1, key 3, value column 40 (head 1)
    qkv_k[pb] = _poisoned(qkv_k[pb], pk, pc, kind)
    keep = torch.ones(B, Sk)
    keep[:, -1] = 0
    mask = (1.0 - keep) * -10000.0
    qd, kd = qkv_q.to(DEV), qkv_k.to(DEV)
    out, _ = ops16.attention_fwd(qd[..., :H], kd[..., H:2 * H], kd[..., 2 * H:], mask.to(DEV), heads)
    q = qkv_q[..., :H].double().view(B, Sq, heads, d).transpose(1, 2)
    k = qkv_k[..., H:2 * H].double().view(B, Sk, heads, d).transpose(1, 2)
    v = qkv_k[..., 2 * H:].double().view(B, Sk, heads, d).transpose(1, 2)
    p = torch.softmax(q @ k.transpose(-1, -2) / d ** 0.5 + mask.double()[:, None, None, :], -1)
    want = (p @ v).transpose(1, 2).reshape(B, Sq, H)
    vmag = torch.where(torch.isfinite(v), v.abs(), torch.zeros_like(v))
    mag = (p @ vmag).transpose(1, 2).reshape(B, Sq, H)
    bad = ~torch.isfinite(want)
    assert bad[pb, :, 40].all() and int(bad.sum()) == Sq
    _close16_where_finite(out, want, mag, "context, poisoned v", Sq, extra64=2.0 ** -8 * mag)
