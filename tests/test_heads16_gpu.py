"""The bf16 head kernels (csrc/heads16.hip, include/vilbert_hip_heads.h), called directly through vilbert._native.lib() with raw
pointers, and the linears built on them (vilbert.functional.linear on a bf16 input: ragged output widths, GELU / ReLU
under autograd).

Rules of this file (those of tests/test_bf16_helpers_gpu.py): every output starts as NaN patterns / canary bytes and lies
between two canary margins that are checked afterwards; where a kernel writes a rectangle inside a wider buffer the whole
buffer is compared with an image built on the CPU. Row moves and conversions are compared bit for bit; GEMM results against
float64 products of the same bf16 values with helpers.close16 (fp32 accumulation 3e-6 sum|terms| + 1e-5, plus one bf16
rounding |want| / 256 for a bf16 result)."""
import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
CANARY = 0x5A
CANARY16 = 0x5A5A
NAN16 = 0x7fc1


def _lib():
    from vilbert import _native
    return _native.lib()


def _st():
    from vilbert import _native
    return _native.stream_ptr()


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


class Guard:
    """n elements of `dtype` on the device between two canary margins; the payload starts as `fill` (uint16 pattern, bf16
    buffers: a NaN) or as canary bytes."""
    MARGIN = 512

    def __init__(self, n, dtype, fill16=None):
        self.nbytes = n * torch.empty((), dtype=dtype).element_size()
        self.buf = torch.full((2 * self.MARGIN + self.nbytes,), CANARY, dtype=torch.uint8, device=DEV)
        self.t = self.buf[self.MARGIN:self.MARGIN + self.nbytes].view(dtype)
        assert self.t.data_ptr() % 16 == 0
        if fill16 is not None:
            self.t.view(torch.int16).fill_(int(np.array(fill16, dtype=np.uint16).view(np.int16)))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        torch.cuda.synchronize()
        m = self.MARGIN
        assert bool((self.buf[:m] == CANARY).all()) and bool((self.buf[m + self.nbytes:] == CANARY).all()), \
            "%s: wrote outside its buffer" % what

    def u16(self, what):
        self.check(what)
        return self.t.view(torch.int16).cpu().numpy().view(np.uint16)

    def f32(self, what):
        self.check(what)
        return self.t.cpu()


def _bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _bf16_from_bits(bits16):
    return torch.from_numpy(np.ascontiguousarray(bits16).view(np.int16).copy()).view(BF16)


def _f32_from_bits(bits32):
    return torch.from_numpy(np.ascontiguousarray(bits32).view(np.int32).copy()).view(torch.float32)


def _random_bf16_bits(rows, cols, seed):
    """every bit pattern class, NaN / Inf / subnormals / -0 included: a row move must not touch a bit"""
    rng = np.random.RandomState(seed)
    return rng.randint(0, 1 << 16, size=(rows, cols)).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------------
# gather / invert / scatter
# ---------------------------------------------------------------------------------------------------------------------
def _map_for(M, src_rows, seed):
    """a row map as _row_map builds it, plus what a caller might get wrong: distinct source rows, a row 0 entry, -1 padding,
    entries below and beyond the source"""
    rng = np.random.RandomState(seed)
    take = min(src_rows, max(1, (M + 1) // 2))
    m = np.full(M, -1, dtype=np.int32)
    rows = rng.permutation(src_rows)[:take]
    if 0 not in rows:
        rows[0] = 0
    slots = rng.permutation(M)[:take]
    m[slots] = rows[:len(slots)]
    free = np.flatnonzero(m == -1)
    for k, bad in zip(free[:3], (src_rows, -7, src_rows + 1000)):
        m[k] = bad
    return m


@pytest.mark.parametrize("M", [1, 33, 96])
@pytest.mark.parametrize("cols", [8, 256, 1024])
def test_gather_and_scatter_move_rows_bit_for_bit(M, cols):
    _check_gather_and_scatter(M, cols, lds=cols + 16, ldo=cols + 8, ldf=cols + 24)


def test_gather_and_scatter_move_dense_rows_bit_for_bit():
    """lds == ldo == cols: the form the fp32 block rows take through the same mover (csrc/rowmap.hip)"""
    _check_gather_and_scatter(33, 8, lds=8, ldo=8, ldf=8)


def _check_gather_and_scatter(M, cols, lds, ldo, ldf):
    lib = _lib()
    src_rows = 50
    bits = _random_bf16_bits(src_rows, lds, seed=M * 7 + cols)
    src = torch.from_numpy(bits.view(np.int16)).to(DEV)
    m = _map_for(M, src_rows, seed=M + cols)
    dmap = torch.from_numpy(m).to(DEV)
    out = Guard(M * ldo, BF16, fill16=NAN16)
    assert lib.vbh_gather_rows_bf16(_st(), M, cols, src.data_ptr(), lds, src_rows, dmap.data_ptr(), out.ptr, ldo) == 0
    got = out.u16("gather").reshape(M, ldo)
    inside = (m >= 0) & (m < src_rows)
    want = np.full((M, ldo), NAN16, dtype=np.uint16)                    # the stride gap is not touched
    want[:, :cols] = 0
    want[inside, :cols] = bits[m[inside], :cols]                        # = index_select on the named rows
    assert (got == want).all(), "gather"
    sel = torch.from_numpy(bits[:, :cols].view(np.int16)).index_select(0, torch.from_numpy(m[inside].astype(np.int64)))
    assert (got[inside, :cols].view(np.int16) == sel.numpy()).all()

    # scatter: every row of `full` is its compact row or +0 - written once, no fill in front (the buffer starts as NaN)
    inv = Guard(src_rows, torch.int32)
    full = Guard(src_rows * ldf, BF16, fill16=NAN16)
    compact = torch.from_numpy(got.view(np.int16).copy()).to(DEV)        # the gathered block, row stride ldo
    assert lib.vbh_invert_map(_st(), src_rows, M, dmap.data_ptr(), inv.ptr) == 0
    assert lib.vbh_scatter_rows_bf16(_st(), src_rows, cols, compact.data_ptr(), ldo, M, inv.ptr, full.ptr, ldf) == 0
    inv.check("invert")
    got_inv = inv.t.cpu().numpy()
    want_inv = np.full(src_rows, -1, dtype=np.int32)
    for r in range(M - 1, -1, -1):                                      # the first entry that names a row wins
        if inside[r]:
            want_inv[m[r]] = r
    assert (got_inv == want_inv).all(), "invert"
    f = full.u16("scatter").reshape(src_rows, ldf)
    want_f = np.full((src_rows, ldf), NAN16, dtype=np.uint16)
    want_f[:, :cols] = 0
    named = want_inv >= 0
    want_f[named, :cols] = bits[named, :cols]
    assert (f == want_f).all(), "scatter"
    # gather(scatter(x)) == x on the named rows
    back = Guard(M * cols, BF16, fill16=NAN16)
    assert lib.vbh_gather_rows_bf16(_st(), M, cols, full.ptr, ldf, src_rows, dmap.data_ptr(), back.ptr, cols) == 0
    assert (back.u16("gather of the scatter").reshape(M, cols) == got[:, :cols]).all()


def test_scatter_with_no_compact_rows_writes_zeros_and_the_wrappers_agree():
    from vilbert import ops16
    lib = _lib()
    inv = Guard(5, torch.int32)
    full = Guard(5 * 8, BF16, fill16=NAN16)
    assert lib.vbh_invert_map(_st(), 5, 0, None, inv.ptr) == 0
    assert lib.vbh_scatter_rows_bf16(_st(), 5, 8, None, 8, 0, inv.ptr, full.ptr, 8) == 0
    assert (inv.t.cpu().numpy() == -1).all() and (full.u16("empty scatter") == 0).all()
    x = _rand(40, 64, seed=3).to(BF16).to(DEV)
    m = torch.tensor([0, 36, -1, 7, 39, -1, 12, -1], dtype=torch.int32, device=DEV)
    g = ops16.gather_rows(x.view(10, 4, 64)[:, 0], m[:2] // 4)          # a row-strided view: row 0 of every sample
    assert torch.equal(g, x[[0, 36]])
    c = ops16.gather_rows(x, m)
    assert torch.equal(c[[0, 1, 3, 4, 6]], x[[0, 36, 7, 39, 12]]) and not c[[2, 5, 7]].any()
    f = ops16.scatter_rows(c, m, 40)
    keep = torch.zeros(40, dtype=torch.bool)
    keep[[0, 36, 7, 39, 12]] = True
    assert torch.equal(f[keep.to(DEV)], x[keep.to(DEV)]) and not f[(~keep).to(DEV)].any()


# ---------------------------------------------------------------------------------------------------------------------
# zero-padded weight shadow
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 211, 1601])
@pytest.mark.parametrize("K", [128, 768])
def test_ragged_shadow_rounds_like_torch_and_pads_with_zeros(n, K):
    lib = _lib()
    n_pad = int(lib.vbh_padded(n))
    assert n_pad % 256 == 0 and 0 <= n_pad - n < 256
    ldw = K + 4
    pats = helpers.rounding_patterns()
    rng = np.random.RandomState(n + K)
    bits = rng.randint(0, 1 << 32, size=(n, ldw), dtype=np.uint64).astype(np.uint32)
    take = min(pats.size, n * K)                                       # every rounding decision (NaN, Inf, subnormals) first
    flat = bits[:, :K].reshape(-1)
    flat[:take] = pats[rng.permutation(pats.size)[:take]]
    bits[:, :K] = flat.reshape(n, K)
    w = _f32_from_bits(bits).to(DEV)
    bias = _rand(n, seed=n).to(DEV)
    w16 = Guard(n_pad * K, BF16, fill16=NAN16)
    wt16 = Guard(K * n_pad, BF16, fill16=NAN16)
    bpad = Guard(n_pad, torch.float32)
    assert lib.vbh_weight_shadow_ragged(_st(), n, K, w.data_ptr(), ldw, bias.data_ptr(), w16.ptr, wt16.ptr, bpad.ptr) == 0
    got = w16.u16("w16").reshape(n_pad, K)
    helpers.check_rounding_contract(bits[:, :K], got[:n], "ragged shadow")
    assert (got[n:] == 0).all(), "pad rows"
    assert (wt16.u16("wt16").reshape(K, n_pad) == got.T).all(), "transpose"
    b = bpad.f32("bias")
    assert torch.equal(b[:n], bias.cpu()) and not b[n:].any()
    # either output alone, and no bias
    only = Guard(K * n_pad, BF16, fill16=NAN16)
    b0 = Guard(n_pad, torch.float32)
    assert lib.vbh_weight_shadow_ragged(_st(), n, K, w.data_ptr(), ldw, None, None, only.ptr, b0.ptr) == 0
    assert (only.u16("wt16 alone").reshape(K, n_pad) == got.T).all() and not b0.f32("no bias").any()


# ---------------------------------------------------------------------------------------------------------------------
# loss backwards
# ---------------------------------------------------------------------------------------------------------------------
def _loss_case(rows, n, seed):
    ld = n + (4 - n % 4) % 4 + 4 if seed % 2 else n                     # padded rows (16-byte loads) and dense rows
    buf = torch.zeros(rows, ld)
    buf[:, :n] = _rand(rows, n, seed=seed, scale=3.0)
    labels = torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(seed))
    labels[::3] = -1                                                    # ignored rows (row 0 among them)
    if rows > 1:
        labels[1] = n - 1
    return buf.to(DEV), ld, labels.to(DEV)


@pytest.mark.parametrize("rows", [1, 5, 64, 65, 70])      # 64, 65: exactly one row tile, one tile + a single row
@pytest.mark.parametrize("n", [2, 211, 1601])
def test_cross_entropy_backward_emits_the_cast_of_the_fp32_gradient_and_its_transpose(rows, n):
    from vilbert import ops
    lib = _lib()
    logits, ld, labels = _loss_case(rows, n, seed=rows + n)
    if rows == 5:
        labels[:] = torch.tensor([3 % n, -1, n - 1, 0, -1])
    view = logits[:, :n]
    _loss, lse, count = ops.xent_fwd(view, labels, -1)
    gl = torch.full((1,), 0.7, device=DEV)
    want = ops.xent_bwd(gl, view, labels, -1, lse, count).to(BF16)      # torch's cast of the fp32 kernel's gradient
    n_pad, m_pad = int(lib.vbh_padded(n)), int(lib.vbh_padded(rows))
    ldg, ldgt = n_pad + 8, m_pad + 16
    G = Guard(rows * ldg, BF16, fill16=NAN16)
    GT = Guard(n_pad * ldgt, BF16, fill16=NAN16)
    parts = int(lib.vbh_colsum_parts_count(rows))
    assert parts == (rows + 63) // 64
    part = Guard(parts * n_pad, torch.float32)
    assert lib.vbh_xent_bwd_bf16(_st(), rows, n, logits.data_ptr(), ld, labels.data_ptr(), -1, lse.data_ptr(), gl.data_ptr(),
                                 count.data_ptr(), G.ptr, ldg, GT.ptr, ldgt, part.ptr) == 0
    g = G.u16("G").reshape(rows, ldg)
    img = np.full((rows, ldg), NAN16, dtype=np.uint16)
    img[:, :n_pad] = 0                                                  # +0 in the pad columns and the ignored rows
    img[:, :n] = _bits16(want)
    assert (g == img).all(), "G"
    ignored = (labels == -1).cpu().numpy()
    assert ignored.any() and (g[ignored, :n_pad] == 0).all()
    gt = GT.u16("GT").reshape(n_pad, ldgt)
    img_t = np.full((n_pad, ldgt), NAN16, dtype=np.uint16)
    img_t[:, :m_pad] = 0
    img_t[:, :rows] = img[:, :n_pad].T
    assert (gt == img_t).all(), "GT"
    # the fp32 column sums per 64 rows of the UNROUNDED gradient: fp32 sums of at most 64 fp32 terms in another order than
    # the reference's float64 sum of the same fp32 values - 64 x 2^-24 sum|terms|
    d32 = ops.xent_bwd(gl, view, labels, -1, lse, count).cpu().double()
    if rows > 1 or labels[0] != -1:
        pt = part.f32("column-sum partials").reshape(parts, n_pad)
        assert not pt[:, n:].any(), "pad columns of the partials"
        for p in range(parts):
            blk = d32[64 * p:64 * p + 64]
            err = (pt[p, :n].double() - blk.sum(0)).abs()
            assert (err <= 64 * 2.0 ** -24 * blk.abs().sum(0) + 1e-30).all(), ("partials", p, float(err.max()))
        # second stage: added into the target in row order - additions only, so the CPU restatement is bit-equal
        init = _rand(n, seed=9)
        out = Guard(n, torch.float32)
        out.t.copy_(init)
        assert lib.vbh_colsum_parts(_st(), parts, n, part.ptr, n_pad, out.ptr) == 0
        acc = torch.zeros(n)
        for p in range(parts):
            acc = acc + pt[p, :n]
        assert torch.equal(out.f32("column sums"), init + acc)
    # G alone, and G with the partials but without GT
    G2 = Guard(rows * n_pad, BF16, fill16=NAN16)
    assert lib.vbh_xent_bwd_bf16(_st(), rows, n, logits.data_ptr(), ld, labels.data_ptr(), -1, lse.data_ptr(), gl.data_ptr(),
                                 count.data_ptr(), G2.ptr, n_pad, None, 0, None) == 0
    assert (G2.u16("G alone").reshape(rows, n_pad) == img[:, :n_pad]).all()
    G3, part3 = Guard(rows * n_pad, BF16, fill16=NAN16), Guard(parts * n_pad, torch.float32)
    assert lib.vbh_xent_bwd_bf16(_st(), rows, n, logits.data_ptr(), ld, labels.data_ptr(), -1, lse.data_ptr(), gl.data_ptr(),
                                 count.data_ptr(), G3.ptr, n_pad, None, 0, part3.ptr) == 0
    assert (G3.u16("G + partials").reshape(rows, n_pad) == img[:, :n_pad]).all()
    assert torch.equal(part3.f32("partials without GT").view(torch.int32), part.f32("partials").view(torch.int32))


@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("n", [2, 211, 1601])
def test_kl_backward_emits_the_cast_of_the_fp32_gradient(rows, n):
    from vilbert import ops
    lib = _lib()
    scores = _rand(rows, n, seed=rows * 3 + n, scale=2.0).to(DEV)
    target = torch.softmax(_rand(rows, n, seed=n), dim=1)
    target[::4] = 0.0                                                   # padding rows of the fixed-capacity gather
    target = target.to(DEV)
    for divisor in (float(rows), torch.full((1,), 3.0, device=DEV)):
        _loss, lse, tsum = ops.kl_fwd(scores, target, divisor)
        gl = torch.full((1,), 1.3, device=DEV)
        want = ops.kl_bwd(gl, scores, target, lse, tsum, divisor).to(BF16)
        n_pad = int(lib.vbh_padded(n))
        ldg = n_pad + 8
        G = Guard(rows * ldg, BF16, fill16=NAN16)
        dev_div = divisor.data_ptr() if torch.is_tensor(divisor) else None
        assert lib.vbh_kl_bwd_bf16(_st(), rows, n, scores.data_ptr(), n, target.data_ptr(), n, lse.data_ptr(), tsum.data_ptr(),
                                   gl.data_ptr(), 0.0 if torch.is_tensor(divisor) else divisor, dev_div, G.ptr, ldg) == 0
        img = np.full((rows, ldg), NAN16, dtype=np.uint16)
        img[:, :n_pad] = 0
        img[:, :n] = _bits16(want)
        assert (G.u16("G") .reshape(rows, ldg) == img).all(), "KL G"


# ---------------------------------------------------------------------------------------------------------------------
# activation backwards
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(1, 8), (4, 1024), (37, 264)])
def test_pooler_relu_backward_is_the_cast_of_the_masked_gradient(rows, cols):
    lib = _lib()
    ldd, ldy, ldo = cols + 4, cols + 8, cols + 8
    dy = _rand(rows, ldd, seed=rows, scale=2.0)
    y = torch.relu(_rand(rows, ldy, seed=cols))
    dy[0, :8] = torch.tensor([float("inf"), -1.0, float("nan"), -0.0, 1e-40, -3.0, 2.0, float("-inf")])
    y[0, :8] = torch.tensor([0.0, 0.0, 1.0, 1.0, 1e-40, -0.0, 5.0, 2.0])
    out = Guard(rows * ldo, BF16, fill16=NAN16)
    dyd, yd = dy.to(DEV), y.to(DEV)
    assert lib.vbh_relu_bwd_bf16(_st(), rows, cols, dyd.data_ptr(), ldd, yd.data_ptr(), ldy, out.ptr, ldo) == 0
    want = (dy[:, :cols] * (y[:, :cols] > 0)).to(BF16)
    got = out.u16("relu backward").reshape(rows, ldo)
    wb = _bits16(want)
    nan = torch.isnan(want.float()).numpy()
    assert ((got[:, :cols] == wb) | nan).all() and ((got[:, :cols] & 0x7fff) > 0x7f80)[nan].all()
    assert (got[:, cols:] == NAN16).all()


@pytest.mark.parametrize("rows,cols", [(1, 8), (37, 264), (5, 1024)])
def test_gelu_backward_multiply_rounds_the_fp32_product_once(rows, cols):
    lib = _lib()
    lda, ldb, ldo = cols + 8, cols + 16, cols + 8
    a = _rand(rows, lda, seed=rows + 1, scale=2.0).to(BF16)
    b = _rand(rows, ldb, seed=cols + 1).to(BF16)
    out = Guard(rows * ldo, BF16, fill16=NAN16)
    ad, bd = a.to(DEV), b.to(DEV)
    assert lib.vbh_mul_bf16(_st(), rows, cols, ad.data_ptr(), lda, bd.data_ptr(), ldb, out.ptr, ldo) == 0
    want = (a[:, :cols].float() * b[:, :cols].float()).to(BF16)           # the product of two bf16 values is exact in fp32
    got = out.u16("mul").reshape(rows, ldo)
    assert (got[:, :cols] == _bits16(want)).all() and (got[:, cols:] == NAN16).all()


# ---------------------------------------------------------------------------------------------------------------------
# functional.linear on a bf16 input: ragged output widths, GELU / ReLU under autograd
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def bf16_mode():
    from vilbert import _native
    prev = _native.set_gemm_mode("bf16")
    yield
    _native.set_gemm_mode(prev)


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _census(monkeypatch):
    """names of the fp32-tensor launchers and casts a piece of code goes through"""
    from vilbert import ops, ops16
    seen = []
    for mod, name in ((ops, "linear_fwd"), (ops, "linear_bwd_input"), (ops, "linear_bwd_weight"), (ops, "xent_bwd"),
                      (ops, "kl_bwd"), (ops, "act_bwd"), (ops16, "cast_f32"), (ops16, "linear_bwd_weight_ragged")):
        orig = getattr(mod, name)
        monkeypatch.setattr(mod, name, (lambda o, n: lambda *a, **k: (seen.append(n), o(*a, **k))[1])(orig, name))
    return seen


@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("K", [128, 768])
@pytest.mark.parametrize("n", [2, 211, 1601])
def test_ragged_linear_under_autograd_matches_float64_on_the_bf16_operands(bf16_mode, monkeypatch, n, K, rows):
    from vilbert import functional as F, ops, ops16
    x16 = _rand(rows, K, seed=n + rows).to(BF16)
    w32, b32 = _rand(n, K, seed=K + n, scale=0.05), _rand(n, seed=7)
    x, w, b = _leaf(x16), _leaf(w32), _leaf(b32)
    seen = _census(monkeypatch)
    y = F.linear(x, w, b, out_f32=True)
    assert y.dtype == torch.float32 and y.shape == (rows, n) and y.stride(0) == ops16.padded(n)
    w64, x64 = w32.to(BF16).double(), x16.double()
    helpers.close16(y, x64 @ w64.t() + b32.double(), x64.abs() @ w64.abs().t() + b32.abs().double(), "ragged forward")
    labels = torch.randint(0, n, (rows,), generator=torch.Generator().manual_seed(rows)).to(DEV)
    labels[::5] = -1
    if rows == 1:
        labels[0] = n - 1
    F.cross_entropy(y, labels, ignore_index=-1).backward()
    torch.cuda.synchronize()
    assert seen == [], seen                                             # no fp32-tensor GEMM, loss backward or cast
    # the operands of the three backward GEMMs: the bf16 loss gradient (held to the fp32 kernel bit for bit above)
    _loss, lse, count = ops.xent_fwd(y.detach(), labels, -1)
    one = torch.ones(1, device=DEV)
    G, GT = ops16.xent_bwd16(one, y.detach(), labels, -1, lse, count, True)
    g64 = G[:, :n].cpu().double()
    dx64, dx_mag = g64 @ w64, g64.abs() @ w64.abs()
    helpers.close16(x.grad, dx64, dx_mag, "ragged dX")
    helpers.close16(w.grad, g64.t() @ x64, g64.abs().t() @ x64.abs(), "ragged dW")
    # the bias gradient does not come from the rounded G: fp32 column sums of the fp32 loss gradient (vbh_colsum_parts)
    d64 = ops.xent_bwd(one, y.detach(), labels, -1, lse, count).cpu().double()
    helpers.close16(b.grad, d64.sum(0), d64.abs().sum(0), "ragged db")
    # both forms of the input gradient, against the same float64 value
    with torch.no_grad():
        for form in ("dgrad", "wgrad"):
            helpers.close16(ops16.linear_ragged_bwd_input(G, GT, w, b, rows, form=form), dx64, dx_mag, "dX, form " + form)


def test_ragged_linear_takes_an_fp32_gradient_from_any_other_consumer(bf16_mode):
    from vilbert import functional as F
    rows, n, K = 77, 211, 128
    x16, dy = _rand(rows, K, seed=1).to(BF16), _rand(rows, n, seed=2)
    w32, b32 = _rand(n, K, seed=3, scale=0.05), _rand(n, seed=4)
    x, w, b = _leaf(x16), _leaf(w32), _leaf(b32)
    y = F.linear(x, w, b, out_f32=True)
    (y * 1.0).backward(dy.to(DEV))                                      # through another node: a plain fp32 gradient
    g64, w64, x64 = dy.to(BF16).double(), w32.to(BF16).double(), x16.double()
    helpers.close16(x.grad, g64 @ w64, g64.abs() @ w64.abs(), "dX")
    helpers.close16(w.grad, g64.t() @ x64, g64.abs().t() @ x64.abs(), "dW")
    helpers.close16(b.grad, g64.sum(0), g64.abs().sum(0), "db")
    # and a loss on logits of an fp32 linear still hands out its fp32 gradient
    z = _leaf(_rand(5, 211, seed=5))
    F.cross_entropy(z, torch.tensor([0, 3, -1, 210, 7], device=DEV), ignore_index=-1).backward()
    assert z.grad.dtype == torch.float32 and bool(torch.isfinite(z.grad).all()) and not z.grad[2].any()


def test_kl_loss_hands_its_bf16_gradient_to_the_region_decoder(bf16_mode, monkeypatch):
    from vilbert import functional as F, ops, ops16
    rows, n, K = 37, 1601, 128
    x16 = _rand(rows, K, seed=11).to(BF16)
    w32, b32 = _rand(n, K, seed=12, scale=0.05), _rand(n, seed=13)
    target = torch.softmax(_rand(rows, n, seed=14), dim=1).to(DEV)
    x, w, b = _leaf(x16), _leaf(w32), _leaf(b32)
    seen = _census(monkeypatch)
    y = F.linear(x, w, b, out_f32=True)
    F.kl_div_log_softmax(y, target, float(rows)).backward()
    torch.cuda.synchronize()
    assert seen == [], seen
    _loss, lse, tsum = ops.kl_fwd(y.detach(), target, float(rows))
    G = ops16.kl_bwd16(torch.ones(1, device=DEV), y.detach(), target, lse, tsum, float(rows))
    g64, w64, x64 = G[:, :n].cpu().double(), w32.to(BF16).double(), x16.double()
    helpers.close16(x.grad, g64 @ w64, g64.abs() @ w64.abs(), "dX")
    helpers.close16(w.grad, g64.t() @ x64, g64.abs().t() @ x64.abs(), "dW")
    helpers.close16(b.grad, g64.sum(0), g64.abs().sum(0), "db")


@pytest.mark.parametrize("rows", [1, 77])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_activation_linear_under_autograd_stays_on_the_bf16_kernels(bf16_mode, monkeypatch, act, rows):
    """GELU (bf16 result, the prediction-head transforms) saves gelu' and multiplies it in backward; ReLU (fp32 result, the
    poolers) masks by its output. The reference takes the bf16 operands the backward GEMMs see: dpre = bf16(dy * gelu') from
    the derivative the forward kernel stores (the same launch, called directly), or bf16(dy * (y > 0)) from the GPU's y."""
    from vilbert import functional as F, ops16
    n, K = 256, 128
    x16 = _rand(rows, K, seed=rows).to(BF16)
    w32, b32 = _rand(n, K, seed=21, scale=0.1), _rand(n, seed=22, scale=0.5)
    x, w, b = _leaf(x16), _leaf(w32), _leaf(b32)
    seen = _census(monkeypatch)
    out_f32 = act == "relu"
    y = F.linear(x, w, b, act=act, out_f32=out_f32)
    assert y.dtype == (torch.float32 if out_f32 else BF16)
    w64, x64 = w32.to(BF16).double(), x16.double()
    pre64 = x64 @ w64.t() + b32.double()
    mag = x64.abs() @ w64.abs().t() + b32.abs().double()
    if act == "gelu":
        want = pre64 * 0.5 * (1.0 + torch.erf(pre64 / 2.0 ** 0.5))
        dy = _rand(rows, n, seed=23).to(BF16)
        # the kernel's erf polynomial is good to 1.5e-7 (csrc/common.h), inside close16's absolute term
        helpers.close16(y, want, mag, "gelu forward")
        y.backward(dy.to(DEV))
        with torch.no_grad():
            dact = ops16.linear_fwd(x.detach(), [w], [b], "gelu", want_act_grad=True)[1]
        dpre = (dy.float() * dact.cpu().float()).to(BF16).double()
    else:
        helpers.close16(y, torch.relu(pre64), mag, "relu forward")
        dy = _rand(rows, n, seed=24)
        y.backward(dy.to(DEV))
        dpre = (dy * (y.detach().cpu() > 0)).to(BF16).double()
    torch.cuda.synchronize()
    assert seen == [], seen
    helpers.close16(x.grad, dpre @ w64, dpre.abs() @ w64.abs(), act + " dX")
    helpers.close16(w.grad, dpre.t() @ x64, dpre.abs().t() @ x64.abs(), act + " dW")
    helpers.close16(b.grad, dpre.sum(0), dpre.abs().sum(0), act + " db")


def test_the_switch_and_swish_keep_the_fp32_detour(bf16_mode, monkeypatch):
    from vilbert import functional as F, ops16
    x16 = _rand(8, 128, seed=1).to(BF16)
    w32, b32 = _rand(256, 128, seed=2, scale=0.1), _rand(256, seed=3)
    for act, off in (("swish", False), ("gelu", True)):
        prev = ops16.set_heads(not off)
        try:
            x, w, b = _leaf(x16), _leaf(w32), _leaf(b32)
            seen = _census(monkeypatch)
            F.linear(x, w, b, act=act).float().sum().backward()
            assert "linear_fwd" in seen and "act_bwd" in seen, (act, seen)
        finally:
            ops16.set_heads(prev)
            monkeypatch.undo()
    prev = ops16.set_heads(False)
    try:
        x, w, b = _leaf(x16), _leaf(_rand(211, 128, seed=4)), _leaf(_rand(211, seed=5))
        seen = _census(monkeypatch)
        y = F.linear(x, w, b, out_f32=True)
        assert y.is_contiguous() and "linear_fwd" in seen                # today's path: the fp32-tensor kernel between casts
    finally:
        ops16.set_heads(prev)
