"""vb_linear_bf16 and vb_wgrad_bf16 (csrc/gemm_bf16.hip) called directly through the C ABI with everything their contract in
include/vilbert_hip.h allows and no caller passes: every built epilogue, row strides larger than the row width on every
operand, every bias form, n_valid on a single tile, and every argument check. vilbert/ops16.py and csrc/layers.hip only ever
launch them dense (lda = K, ldc = N, ...), with a bias, and - for ReLU - under no_grad at the model's widths, so the tests
that go through them (test_bf16_stream_gpu.py, test_bf16_bench_shapes_gpu.py) see none of this.

Rules of this file:
  * the entry points are called through vilbert._native.lib() with N.LinearBf16Args / N.WgradBf16Args; W is a bf16 matrix
    built here (no shadow cache);
  * every expected value is float64 arithmetic on the CPU on the same bf16 operand values, compared with helpers.close16:
    3e-6 sum|a b| + 1e-5 for the fp32 accumulation, plus one bf16 rounding |want| / 256 for a bf16 output. sum|a b| is the sum
    over the products alone (x a multiplier's magnitude for the `mul` epilogue: the terms of that result are a b mul). ReLU,
    GELU and GELU' are 1-Lipschitz (max |gelu''| = 2 phi(0) = 0.80), so the bound of the pre-activation holds after them;
  * a strided launch runs the same kernel in the same order as the dense launch of the same values, so the two results are
    also required to be BIT-identical (all of vb_linear_bf16; vb_wgrad_bf16 under the deterministic setting). The dense launch
    itself is held to float64 in the same test;
  * canaries: the gap columns of every buffer with ld > width are NaN (bf16 0x7FC0 / fp32 NaN). An input NaN that reaches a
    result fails close16's finiteness assert; every output is followed by canary rows (enough to cover the rows a tile-sized
    store without its row guard would hit) and all gap columns and canary rows must hold the canary bits afterwards: "Rows >=
    M are never stored", "nothing past row n_valid is written". Inputs are allocated with exactly the elements the contract
    says are read: (rows - 1) * ld + width;
  * strides all differ, so a swapped one shows: lda = K + 8, ldw = K + 8 (on another row count), ldc = N + 8, ldc32 = N + 4,
    ldr = ldm = N + 16, ldg = N + 24; weight gradient: ldy = N + 8, ldx = K + 16, ldw = K + 3 with dW[s] one float past a
    16-byte boundary (dW is only 4-byte aligned).

Kernel instantiations gemm_bf16_kernel<OUT, EPI, Cfg> reached through vb_linear_bf16, each at Cfg = HbHalf (shapes 300 x 256 x
128 and 1 x 128 x 64: at most 128 full-size tiles) and Cfg = HbFull (4200 x 1024 x 64: 17 x 8 = 136 tiles) by
test_linear_epilogues[<shape>-<case>]:
    case        instantiation                the epilogue form
    plain       <HB_OUT_BF16, HB_PLAIN>      v = acc + bias
    gelu_grad   <HB_OUT_BF16, HB_GELU>       gelu(v), gelu'(v) to act_grad
    gelu        <HB_OUT_BF16, HB_GELU>       gelu(v), act_grad = NULL
    relu        <HB_OUT_BF16, HB_RELU>       max(v, 0)
    res         <HB_OUT_BF16, HB_RES>        v + residual
    dropres     <HB_OUT_BF16, HB_DROPRES>    dropout(v) + residual, mask index m * N + n
    mul         <HB_OUT_BF16, HB_MUL>        v * mul
    f32_plain   <HB_OUT_F32, HB_PLAIN>
    f32_res     <HB_OUT_F32, HB_RES>
    f32_relu    <HB_OUT_F32, HB_RELU>
(7 bf16-out and 3 fp32-out forms = 9 instantiations per block shape; nothing else is built.)

Two things the ABI itself rules out, so no case exists for them: a bias in more than VB_MAX_SEGMENTS = 4 segments (the
narrowest segment, 32 columns, is therefore reached at N = 128 with 4 segments, and N = 256 gets 4 segments of 64), and an
error return for (N / bias_segments) % 32 != 0 - with N % 128 == 0 and at most 4 segments that dividing evenly every quotient
is a multiple of 32, the check cannot fire.
"""
import ctypes
import functools

import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF16 = torch.bfloat16
E_BADARG, E_ALIGN, E_RANGE, E_SEGMENT = -1, -2, -3, -4
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SWISH = 0, 1, 2, 3
MAX_SEGMENTS = 4
NAN = float("nan")
DROP_P, DROP_SEED = 0.25, 0x5EED5EED5EED


def _N():
    from vilbert import _native
    return _native


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _bits(t):
    """The bit patterns of a bf16 / fp32 tensor as an integer tensor of the same shape."""
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _canary_bits(dtype):
    return int(_bits(torch.full((1,), NAN, dtype=dtype))[0])


def _input(t, ld):
    """CPU matrix t [rows, width] (bf16) -> device buffer of exactly (rows - 1) * ld + width elements, row stride ld, the gap
    columns NaN."""
    rows, width = t.shape
    img = torch.full((rows, ld), NAN, dtype=t.dtype)
    img[:, :width] = t
    return img.reshape(-1)[:(rows - 1) * ld + width].clone().to(DEV)


class Out:
    """Output matrix [rows, width] with row stride ld on the device, followed by `extra` canary rows; everything NaN on entry
    except `init` (CPU [rows, width]: a target that is ADDED into). offset: elements the matrix starts past the allocation
    (an fp32 target that is only 4-byte aligned)."""

    def __init__(self, rows, width, ld, dtype, extra, init=None, offset=0):
        self.rows, self.width, self.ld, self.extra = rows, width, ld, extra
        img = torch.full((rows + extra, ld), NAN, dtype=dtype)
        if init is not None:
            img[:rows, :width] = init
        self.buf = torch.full((offset + img.numel(),), NAN, dtype=dtype, device=DEV)
        self.t = self.buf[offset:].view(rows + extra, ld)
        self.t.copy_(img)
        assert self.buf.data_ptr() % 16 == 0

    @property
    def ptr(self):
        return self.t.data_ptr()

    def result(self, what):
        """The [rows, width] result on the CPU, after checking that every gap column and canary row is untouched."""
        torch.cuda.synchronize()
        h = self.t.cpu()
        can = _canary_bits(h.dtype)
        assert bool((_bits(h)[:self.rows, self.width:] == can).all()), "%s: a gap column was written" % what
        assert bool((_bits(h)[self.rows:] == can).all()), "%s: a row past the last one was written" % what
        return h[:self.rows, :self.width].contiguous()

    def untouched(self, what):
        torch.cuda.synchronize()
        h = self.buf.cpu()
        assert bool((_bits(h) == _canary_bits(h.dtype)).all()), "%s: wrote although it returned an error" % what


def _tile_pad(M):
    """Canary rows after an [M, .] output of vb_linear_bf16: up to the end of a 256-row tile, and three more."""
    return (M + 255) // 256 * 256 - M + 3


# ---------------------------------------------------------------------------------------------------------------------
# vb_linear_bf16
# ---------------------------------------------------------------------------------------------------------------------
class Problem:
    """One (M, N, K) problem: bf16 operands on the CPU, their dense and strided device copies, and the float64 products."""

    def __init__(self, M, N, K, seed=0):
        self.M, self.N, self.K = M, N, K
        self.x = _rand(M, K, seed=seed + 1).to(BF16)
        self.w = _rand(N, K, seed=seed + 2, scale=0.05).to(BF16)
        self.r = _rand(M, N, seed=seed + 3).to(BF16)               # residual or multiplier
        self.bias = _rand(N, seed=seed + 4)                          # N(0, 1): relu(acc) + bias is far from relu(acc + bias)
        self.acc = self.x.double() @ self.w.double().t()
        self.mag = self.x.double().abs() @ self.w.double().abs().t()
        self.strides = {"lda": K + 8, "ldw": K + 8, "ldc": N + 8, "ldc32": N + 4, "ldr": N + 16, "ldm": N + 16, "ldg": N + 24}
        self.dense = {"lda": K, "ldw": K, "ldc": N, "ldc32": N, "ldr": N, "ldm": N, "ldg": N}
        self.dev = {}
        for strided, ld in ((False, self.dense), (True, self.strides)):
            self.dev[strided] = {"x": _input(self.x, ld["lda"]), "w": _input(self.w, ld["ldw"]), "r": _input(self.r, ld["ldr"])}
        self._keep = None

    def keep(self):
        """The dropout keep mask of (DROP_P, DROP_SEED) over element index m * N + n, from the fp32 path's vb_dropout."""
        if self._keep is None:
            from vilbert import ops
            self._keep = ops.dropout(torch.ones(self.M, self.N, device=DEV), DROP_P, DROP_SEED).cpu() != 0
            frac = float(self._keep.float().mean())
            assert self.M * self.N < 4096 or abs(frac - (1 - DROP_P)) < 0.05, frac
        return self._keep


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    return Problem(M, N, K)


def _bias_tensors(bias, form):
    """(bias_segments, [device tensor or None per segment]) for a bias form; each segment a separate allocation.
    form: None = no bias at all; "seg0" = bias_segments 0 (one bias of N values); or a tuple of booleans, one per segment
    (False = a NULL segment)."""
    if form is None:
        return 0, [None]
    if form == "seg0":
        return 0, [bias.clone().to(DEV)]
    seg = bias.numel() // len(form)
    return len(form), [bias[s * seg:(s + 1) * seg].clone().to(DEV) if given else None for s, given in enumerate(form)]


def _bias_vector(bias, form):
    """The float64 bias vector that form adds (zeros in NULL segments)."""
    if form is None:
        return torch.zeros_like(bias, dtype=torch.float64)
    if form == "seg0":
        return bias.double()
    seg = bias.numel() // len(form)
    return torch.cat([bias[s * seg:(s + 1) * seg].double() * (1.0 if given else 0.0) for s, given in enumerate(form)])


EPILOGUES = {  # case -> (fp32 out, act, act_grad, residual, mul, dropout)
    "plain": (False, ACT_NONE, False, False, False, False),
    "gelu_grad": (False, ACT_GELU, True, False, False, False),
    "gelu": (False, ACT_GELU, False, False, False, False),
    "relu": (False, ACT_RELU, False, False, False, False),
    "res": (False, ACT_NONE, False, True, False, False),
    "dropres": (False, ACT_NONE, False, True, False, True),
    "mul": (False, ACT_NONE, False, False, True, False),
    "f32_plain": (True, ACT_NONE, False, False, False, False),
    "f32_res": (True, ACT_NONE, False, True, False, False),
    "f32_relu": (True, ACT_RELU, False, False, False, False),
}


def _launch_linear(pb, case, strided, bias_form, what):
    """One vb_linear_bf16 launch of problem pb: (result, act_grad result or None) on the CPU, canaries checked."""
    N = _N()
    f32, act, want_grad, res, mul, drop = EPILOGUES[case]
    ld, dev = (pb.strides if strided else pb.dense), pb.dev[strided]
    nbias, biases = _bias_tensors(pb.bias, bias_form)
    pad = _tile_pad(pb.M)
    out = Out(pb.M, pb.N, ld["ldc32"] if f32 else ld["ldc"], torch.float32 if f32 else BF16, pad)
    grad = Out(pb.M, pb.N, ld["ldg"], BF16, pad) if want_grad else None
    a = N.LinearBf16Args()
    a.A, a.lda, a.W, a.ldw = dev["x"].data_ptr(), ld["lda"], dev["w"].data_ptr(), ld["ldw"]
    a.bias_segments = nbias
    for s, b in enumerate(biases):
        a.bias[s] = b.data_ptr() if b is not None else None
    if f32:
        a.C32, a.ldc32 = out.ptr, ld["ldc32"]
    else:
        a.C, a.ldc = out.ptr, ld["ldc"]
    if res:
        a.residual, a.ldr = dev["r"].data_ptr(), ld["ldr"]
    if mul:
        a.mul, a.ldm = dev["r"].data_ptr(), ld["ldm"]
    if want_grad:
        a.act_grad, a.ldg = grad.ptr, ld["ldg"]
    a.M, a.N, a.K, a.act = pb.M, pb.N, pb.K, act
    if drop:
        a.dropout_p, a.seed = DROP_P, DROP_SEED
    assert N.lib().vb_linear_bf16(N.stream_ptr(), ctypes.byref(a)) == 0, what
    return out.result(what), grad.result(what + ", act_grad") if want_grad else None


def _expected(pb, case, bias_form):
    """float64 (result, its sum|terms|, act_grad or None) of an epilogue case."""
    _f32, act, want_grad, res, mul, drop = EPILOGUES[case]
    pre = pb.acc + _bias_vector(pb.bias, bias_form)
    mag, want, dgrad = pb.mag, pre, None
    if act == ACT_GELU:
        phi = 0.5 * (1 + torch.erf(pre / 2 ** 0.5))
        want = pre * phi
        if want_grad:
            dgrad = phi + pre * torch.exp(-0.5 * pre * pre) / (2 * torch.pi) ** 0.5
    if act == ACT_RELU:
        want = pre.clamp(min=0)
    if drop:
        want = torch.where(pb.keep(), pre / (1 - DROP_P), torch.zeros_like(pre))
    if res:
        want = want + pb.r.double()
    if mul:
        want, mag = pre * pb.r.double(), pb.mag * pb.r.double().abs()
    return want, mag, dgrad


def _check_linear(pb, case, bias_form, what):
    """Dense and strided launch of one case: both against float64, and the strided result bit-identical to the dense one."""
    want, mag, dgrad = _expected(pb, case, bias_form)
    got = {}
    for strided in (False, True):
        tag = "%s, %s" % (what, "strided" if strided else "dense")
        y, d = _launch_linear(pb, case, strided, bias_form, tag)
        assert y.dtype == (torch.float32 if EPILOGUES[case][0] else BF16)
        helpers.close16(y, want, mag, tag)
        if dgrad is not None:
            helpers.close16(d, dgrad, pb.mag, tag + ": gelu'")
        got[strided] = (y, d)
    assert torch.equal(_bits(got[True][0]), _bits(got[False][0])), "%s: the strided result differs from the dense one" % what
    if dgrad is not None:
        assert torch.equal(_bits(got[True][1]), _bits(got[False][1])), "%s: the strided gelu' differs from the dense one" % what


# half-size blocks (plan_hb: at most 128 full-size tiles): three 128-row tiles, the last with 44 live rows; one row.
# full-size blocks: 17 x 8 = 136 tiles, the last tile row with 104 live rows; K = 64 = one K tile per output tile.
LINEAR_SHAPES = [(300, 256, 128), (1, 128, 64), (4200, 1024, 64)]


@pytest.mark.parametrize("case", list(EPILOGUES))
@pytest.mark.parametrize("M,N,K", LINEAR_SHAPES, ids=lambda v: str(v))
def test_linear_epilogues(M, N, K, case):
    _check_linear(_problem(M, N, K), case, (True,), "%d x %d x %d %s" % (M, N, K, case))


def test_relu_cases_tell_relu_before_the_bias_apart():
    """The ReLU cases above are not vacuous: relu(acc) + bias lies outside the bound of relu(acc + bias) on most elements."""
    for M, N, K in LINEAR_SHAPES:
        pb = _problem(M, N, K)
        want = (pb.acc + pb.bias.double()).clamp(min=0)
        wrong = pb.acc.clamp(min=0) + pb.bias.double()
        tol = 3e-6 * pb.mag + 1e-5 + want.abs() / 256
        assert float(((wrong - want).abs() > tol).double().mean()) > 0.5


# N = 256 on half-size blocks (300 rows) and on full-size blocks (65 x 2 = 130 tiles); the 32-column segments of N = 128 with 4
# segments on half-size blocks and on full-size blocks (129 tiles, the last with 32 live rows)
BIAS_CASES = [(M, 256, K, form) for M, K in ((300, 128), (16500, 64))
              for form in (None, "seg0", (True,), (True, False), (False, True, False, True))]
BIAS_CASES += [(M, 128, 64, form) for M in (300, 32800) for form in ((True, False, True, False), (False, True, True, False))]


@pytest.mark.parametrize("M,N,K,form", BIAS_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_linear_bias_forms(M, N, K, form):
    pb = _problem(M, N, K)
    what = "%d x %d x %d bias %s" % (M, N, K, form)
    _check_linear(pb, "plain", form, what)
    if form is not None and form != "seg0" and not all(form):
        # not vacuous: with the first given segment's values in a NULL segment the result is outside the bound
        seg = N // len(form)
        first = pb.bias[form.index(True) * seg:][:seg].double()
        want, _, _ = _expected(pb, "plain", form)
        s = form.index(False)
        wrong = pb.acc[:, s * seg:(s + 1) * seg] + first
        sl = (slice(None), slice(s * seg, (s + 1) * seg))
        assert float(((wrong - want[sl]).abs() > 3e-6 * pb.mag[sl] + 1e-5 + want[sl].abs() / 256).double().mean()) > 0.5


@pytest.mark.parametrize("kind", ["mul", "res"])
@pytest.mark.parametrize("M,n_out,k_in", [(300, 192, 256), (4200, 128, 1024)], ids=lambda v: str(v))
def test_linear_input_gradient_form(M, n_out, k_in, kind):
    """dX [M][k_in] = dY [M][n_out] Wt^T with the TRANSPOSED weight Wt [k_in][n_out] as the kernel's W and no bias: the
    kernel's N is k_in, its contraction n_out (three / two K tiles per output tile: the K stream runs across output tiles).
    With the saved derivative as multiplier and with a residual gradient."""
    pb = _problem(M, k_in, n_out)                                  # x = dY, w = Wt
    weight = pb.w.t().contiguous()                                 # the layer's weight [n_out][k_in]
    dx = pb.x.double() @ weight.double()
    assert float((dx - pb.acc).abs().max()) < 1e-9                 # (the same sums, perhaps in another order)
    _check_linear(pb, kind, None, "input gradient %d x %d x %d, %s" % (M, k_in, n_out, kind))


def _linear_error_setup():
    """A valid 128 x 128 x 64 launch description on buffers large enough for every variation below, all outputs canaries."""
    N = _N()
    M, Nn, K = 128, 128, 64
    x = torch.zeros(M * (K + 64) + 64, dtype=BF16, device=DEV)
    w = torch.zeros(Nn * (K + 64) + 64, dtype=BF16, device=DEV)
    r = torch.zeros(M * (Nn + 64) + 64, dtype=BF16, device=DEV)
    bias = torch.zeros(Nn + 64, device=DEV)
    c = Out(M, Nn, Nn + 64, BF16, 4)
    c32 = Out(M, Nn, Nn + 64, torch.float32, 4)
    g = Out(M, Nn, Nn + 64, BF16, 4)

    def args(**kw):
        a = N.LinearBf16Args()
        a.A, a.lda, a.W, a.ldw = x.data_ptr(), K, w.data_ptr(), K
        a.bias[0], a.bias_segments = bias.data_ptr(), 1
        a.C, a.ldc = c.ptr, Nn
        a.M, a.N, a.K = M, Nn, K
        for k, v in kw.items():
            if k.startswith("bias") and k != "bias_segments":
                a.bias[int(k[4:])] = v
            else:
                setattr(a, k, v)
        return a

    def rc(**kw):
        return N.lib().vb_linear_bf16(N.stream_ptr(), ctypes.byref(args(**kw)))
    return {"rc": rc, "x": x.data_ptr(), "w": w.data_ptr(), "r": r.data_ptr(), "bias": bias.data_ptr(), "c": c, "c32": c32, "g": g,
            "keep": (x, w, r, bias), "M": M, "N": Nn, "K": K}


def test_linear_error_returns():
    N = _N()
    s = _linear_error_setup()
    rc, c, c32, g, r, Nn, K = s["rc"], s["c"], s["c32"], s["g"], s["r"], s["N"], s["K"]
    f32 = {"C": None, "C32": c32.ptr, "ldc32": Nn}
    # ---- VB_E_BADARG
    assert N.lib().vb_linear_bf16(N.stream_ptr(), None) == E_BADARG
    assert rc(A=None) == E_BADARG and rc(W=None) == E_BADARG
    assert rc(C32=c32.ptr, ldc32=Nn) == E_BADARG                                   # both outputs
    assert rc(C=None) == E_BADARG                                                  # neither
    for dim in ("M", "N", "K"):
        assert rc(**{dim: 0}) == E_BADARG and rc(**{dim: -64 if dim == "K" else -128}) == E_BADARG, dim
    assert rc(residual=r, ldr=Nn, mul=r, ldm=Nn) == E_BADARG
    for act in (ACT_GELU, ACT_RELU):
        assert rc(act=act, residual=r, ldr=Nn) == E_BADARG
        assert rc(act=act, mul=r, ldm=Nn) == E_BADARG
        assert rc(act=act, dropout_p=0.25) == E_BADARG
        assert rc(act=act, residual=r, ldr=Nn, dropout_p=0.25) == E_BADARG
    assert rc(act_grad=g.ptr, ldg=Nn) == E_BADARG                                  # act_grad without GELU
    assert rc(act=ACT_RELU, act_grad=g.ptr, ldg=Nn) == E_BADARG
    assert rc(dropout_p=0.25) == E_BADARG                                          # dropout without a residual
    assert rc(dropout_p=0.25, mul=r, ldm=Nn) == E_BADARG
    for p in (-0.25, 1.0, 1.5, NAN, float("inf")):
        assert rc(dropout_p=p, residual=r, ldr=Nn) == E_BADARG, p
    for act in (ACT_SWISH, 4, -1):
        assert rc(act=act) == E_BADARG, act
    assert rc(act=ACT_GELU, **f32) == E_BADARG                                     # fp32 out: plain / residual / ReLU only
    assert rc(residual=r, ldr=Nn, dropout_p=0.25, **f32) == E_BADARG
    assert rc(mul=r, ldm=Nn, **f32) == E_BADARG
    # ---- VB_E_ALIGN
    for k in (32, 96):
        assert rc(K=k, lda=128, ldw=128) == E_ALIGN, k
    for n in (64, 192):
        assert rc(N=n, ldc=256) == E_ALIGN, n
    for ld in ("lda", "ldw"):
        assert rc(**{ld: K + 4}) == E_ALIGN and rc(**{ld: K + 2}) == E_ALIGN and rc(**{ld: K - 8}) == E_ALIGN, ld
    assert rc(ldc=Nn + 4) == E_ALIGN and rc(ldc=Nn + 2) == E_ALIGN and rc(ldc=Nn - 8) == E_ALIGN      # bf16 out: ldc % 8, 16 bytes
    assert rc(**dict(f32, ldc32=Nn + 2)) == E_ALIGN and rc(**dict(f32, ldc32=Nn - 4)) == E_ALIGN
    for name in ("residual", "mul"):
        ld = "ldr" if name == "residual" else "ldm"
        assert rc(**{name: r, ld: Nn + 4}) == E_ALIGN and rc(**{name: r, ld: Nn - 8}) == E_ALIGN, name
        for off in (2, 8):
            assert rc(**{name: r + off, ld: Nn}) == E_ALIGN, (name, off)
    assert rc(act=ACT_GELU, act_grad=g.ptr, ldg=Nn + 4) == E_ALIGN and rc(act=ACT_GELU, act_grad=g.ptr, ldg=Nn - 8) == E_ALIGN
    for off in (2, 8):
        assert rc(A=s["x"] + off) == E_ALIGN and rc(W=s["w"] + off) == E_ALIGN, off
        assert rc(C=c.ptr + off) == E_ALIGN, off
        assert rc(act=ACT_GELU, act_grad=g.ptr + off, ldg=Nn) == E_ALIGN, off
    for off in (4, 8):
        assert rc(**dict(f32, C32=c32.ptr + off)) == E_ALIGN, off
        assert rc(bias0=s["bias"] + off) == E_ALIGN, off
    assert rc(bias_segments=2, bias1=s["bias"] + 4) == E_ALIGN
    # ---- VB_E_SEGMENT ((N / bias_segments) % 32 != 0 cannot be reached: see the head of the file)
    assert rc(bias_segments=MAX_SEGMENTS + 1) == E_SEGMENT
    assert rc(bias_segments=3) == E_SEGMENT                                        # 128 % 3
    # ---- VB_E_RANGE: the loaders' 32-bit byte offsets hold 256 rows of A / W
    assert rc(lda=1 << 23) == E_RANGE and rc(ldw=1 << 23) == E_RANGE
    for o in (c, c32, g):
        o.untouched("vb_linear_bf16 error returns")


# ---------------------------------------------------------------------------------------------------------------------
# vb_wgrad_bf16
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(params=[True, False], ids=["ordered", "atomics"])
def det(request):
    N = _N()
    wanted = N._DET["wanted"]
    N.set_deterministic(request.param)
    yield request.param
    N.set_deterministic(wanted)


def _launch_wgrad(dy, x, nseg, seg_n, strided, init_w, init_b, n_valid=0, rows=None):
    """One vb_wgrad_bf16 launch: dy [M, nseg seg_n], x [M, K] bf16 on the CPU; init_w[s] [rows, K] / init_b[s] [rows] or None
    (no bias gradient for that segment) the values the targets hold on entry (rows = seg_n, or n_valid where that is given as
    the number of rows that exist). Returns ([dW_s], [dbias_s or None]) on the CPU, canaries checked."""
    N = _N()
    M, K = x.shape
    n = nseg * seg_n
    rows = seg_n if rows is None else rows
    ldy, ldx, ldw, off = (n + 8, K + 16, K + 3, 1) if strided else (n, K, K, 0)
    dyd, xd = _input(dy, ldy), _input(x, ldx)
    pad = seg_n - rows + 3                              # canaries up to the end of the segment's tiles, and three more
    dws = [Out(rows, K, ldw, torch.float32, pad, init=init_w[s], offset=off) for s in range(nseg)]
    dbs = [Out(1, rows, rows + pad, torch.float32, 1, init=init_b[s][None, :]) if init_b[s] is not None else None for s in range(nseg)]
    a = N.WgradBf16Args()
    a.dY, a.ldy, a.X, a.ldx, a.ldw = dyd.data_ptr(), ldy, xd.data_ptr(), ldx, ldw
    a.M, a.K, a.nseg, a.seg_n, a.n_valid = M, K, nseg, seg_n, n_valid
    for s in range(nseg):
        a.dW[s] = dws[s].ptr
        a.dbias[s] = dbs[s].ptr if dbs[s] is not None else None
        assert dws[s].ptr % 16 == 4 * off
    before = N.deterministic_fallbacks()
    assert N.lib().vb_wgrad_bf16(N.stream_ptr(), ctypes.byref(a)) == 0
    assert N.deterministic_fallbacks() == before, "the ordered reduce was wanted and the launch ran with atomics"
    tag = "strided" if strided else "dense"
    return ([o.result("dW %s" % tag) for o in dws],
            [o.result("dbias %s" % tag)[0] if o is not None else None for o in dbs])


def _check_wgrad(got, dy, x, nseg, seg_n, init_w, init_b, what, rows=None):
    rows = seg_n if rows is None else rows
    dws, dbs = got
    for s in range(nseg):
        seg = dy[:, s * seg_n:s * seg_n + rows].double()
        helpers.close16(dws[s], init_w[s].double() + seg.t() @ x.double(), seg.abs().t() @ x.double().abs(), "%s: dW %d" % (what, s))
        if init_b[s] is not None:
            helpers.close16(dbs[s], init_b[s].double() + seg.sum(0), seg.abs().sum(0), "%s: dbias %d" % (what, s))
        else:
            assert dbs[s] is None


def _same_bits(a, b, what):
    for s, (u, v) in enumerate(zip(a[0], b[0])):
        assert torch.equal(_bits(u), _bits(v)), "%s: dW %d" % (what, s)
    for s, (u, v) in enumerate(zip(a[1], b[1])):
        assert (u is None and v is None) or torch.equal(_bits(u), _bits(v)), "%s: dbias %d" % (what, s)


# one output tile (4 contraction tiles of 64 rows, the last with 8); 6 tiles of three stacked segments with a ragged last
# contraction tile of 12 rows (1100 = 17 x 64 + 12)
@pytest.mark.parametrize("M,nseg,seg_n,K", [(200, 1, 256, 128), (1100, 3, 256, 256)], ids=lambda v: str(v))
def test_wgrad_strided_operands_and_targets(det, M, nseg, seg_n, K):
    x, dy = _rand(M, K, seed=1).to(BF16), _rand(M, nseg * seg_n, seed=4).to(BF16)
    init_w = [_rand(seg_n, K, seed=30 + s) for s in range(nseg)]
    init_b = [_rand(seg_n, seed=40 + s) if s % 2 == 0 else None for s in range(nseg)]       # NULL dbias in the odd segments
    what = "wgrad %d x %d x %d x %d" % (M, nseg, seg_n, K)
    dense = _launch_wgrad(dy, x, nseg, seg_n, False, init_w, init_b)
    _check_wgrad(dense, dy, x, nseg, seg_n, init_w, init_b, what + " dense")
    strided = _launch_wgrad(dy, x, nseg, seg_n, True, init_w, init_b)
    _check_wgrad(strided, dy, x, nseg, seg_n, init_w, init_b, what + " strided")
    if det:
        _same_bits(strided, dense, what + ": strided differs from dense")
        _same_bits(_launch_wgrad(dy, x, nseg, seg_n, True, init_w, init_b), strided, what + ": two strided runs differ")


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("n_valid", [200, 0, 256])
def test_wgrad_n_valid_on_one_tile(det, n_valid, strided):
    """nseg = 1, seg_n = 256, one output tile: the row guard is the whole launch. n_valid = 200: dY has zero columns past 200,
    dW has 200 rows and dbias 200 entries, each followed by canaries; n_valid = 0 and n_valid = seg_n give the full result."""
    M, seg_n, K = 200, 256, 128
    rows = n_valid if n_valid else seg_n
    x, dy = _rand(M, K, seed=5).to(BF16), _rand(M, seg_n, seed=6).to(BF16)
    dy[:, rows:] = 0
    init_w, init_b = [_rand(rows, K, seed=7)], [_rand(rows, seed=8)]
    what = "wgrad n_valid = %d" % n_valid
    got = _launch_wgrad(dy, x, 1, seg_n, strided, init_w, init_b, n_valid=n_valid, rows=rows)
    _check_wgrad(got, dy, x, 1, seg_n, init_w, init_b, what, rows=rows)
    if det:
        _same_bits(_launch_wgrad(dy, x, 1, seg_n, strided, init_w, init_b, n_valid=n_valid, rows=rows), got, what + ": two runs differ")


def test_wgrad_error_returns(det):
    N = _N()
    M, seg_n, K = 64, 256, 128
    x = torch.zeros(M * (K + 64) + 64, dtype=BF16, device=DEV)
    dy = torch.zeros(M * (2 * seg_n + 64) + 64, dtype=BF16, device=DEV)
    dws = [Out(seg_n, K, K + 8, torch.float32, 4) for _ in range(2)]
    dbs = [Out(1, seg_n, seg_n + 8, torch.float32, 1) for _ in range(2)]

    def rc(**kw):
        a = N.WgradBf16Args()
        a.dY, a.ldy, a.X, a.ldx, a.ldw = dy.data_ptr(), seg_n, x.data_ptr(), K, K
        a.M, a.K, a.nseg, a.seg_n = M, K, 1, seg_n
        for s in range(2):
            a.dW[s], a.dbias[s] = dws[s].ptr, dbs[s].ptr
        for k, v in kw.items():
            if k in ("dW0", "dW1"):
                a.dW[int(k[2])] = v
            else:
                setattr(a, k, v)
        return N.lib().vb_wgrad_bf16(N.stream_ptr(), ctypes.byref(a))
    two = {"nseg": 2, "ldy": 2 * seg_n}
    # ---- VB_E_BADARG
    assert N.lib().vb_wgrad_bf16(N.stream_ptr(), None) == E_BADARG
    assert rc(dY=None) == E_BADARG and rc(X=None) == E_BADARG
    for name, bad in (("M", (0, -64)), ("K", (0, -128)), ("nseg", (0, -1, MAX_SEGMENTS + 1)), ("seg_n", (0, -256))):
        for v in bad:
            assert rc(**{name: v}) == E_BADARG, (name, v)
    assert rc(dW0=None) == E_BADARG and rc(dW1=None, **two) == E_BADARG
    assert rc(dW0=dws[0].ptr + 2) == E_BADARG and rc(dW1=dws[1].ptr + 2, **two) == E_BADARG
    assert rc(n_valid=-1) == E_BADARG and rc(n_valid=seg_n + 1) == E_BADARG
    assert rc(n_valid=200, **two) == E_BADARG                                      # a partial n_valid needs nseg == 1
    # ---- VB_E_ALIGN
    for v in (128, 384):
        assert rc(seg_n=v, ldy=512) == E_ALIGN, v
    for v in (64, 192):
        assert rc(K=v, ldx=256, ldw=256) == E_ALIGN, v
    assert rc(ldy=seg_n + 4) == E_ALIGN and rc(ldy=seg_n - 8) == E_ALIGN and rc(nseg=2) == E_ALIGN     # ldy < nseg seg_n
    assert rc(ldx=K + 4) == E_ALIGN and rc(ldx=K - 8) == E_ALIGN
    assert rc(ldw=K - 1) == E_ALIGN
    for off in (2, 8):
        assert rc(dY=dy.data_ptr() + off) == E_ALIGN and rc(X=x.data_ptr() + off) == E_ALIGN, off
    # ---- VB_E_RANGE: the loaders' 32-bit byte offsets hold the 64 rows of a contraction tile
    assert rc(ldy=1 << 25) == E_RANGE and rc(ldx=1 << 25) == E_RANGE
    for o in dws + dbs:
        o.untouched("vb_wgrad_bf16 error returns")
