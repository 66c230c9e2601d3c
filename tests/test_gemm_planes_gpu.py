"""vb_linear_fwd, vb_linear_bwd_input and vb_linear_bwd_weight (csrc/gemm.hip) called directly through the C ABI in every
process-wide GEMM mode: "bf16x6" / "bf16x3" / "bf16" (csrc/gemm_planes.hip with 3 / 2 / 1 bf16 planes: launch_gemm skips every
planner there, so forward, input gradient and weight gradient of every shape run on gemm_planes_kernel and end in
tile_epilogue, csrc/gemm_core.h) and "f32" as the control (whichever kernel the planners pick; the fp32 entry points' first
strided and guarded launches).

Rules of this file (those of tests/test_bf16_gemm_abi_gpu.py, whose _input / Out / canary helpers it imports):
  * the entry points are called through vilbert._native.lib() with the ctypes mirrors N.LinearArgs / N.LinearBwdInputArgs /
    N.LinearBwdWeightArgs;
  * every expected value is float64 arithmetic on the CPU, held to the project's own tolerance of tests/test_gemm_modes_gpu.py
    (_check): |got - want| <= 3e-5 (f32, bf16x6) / 6e-4 (bf16x3) / 2^-6 (bf16) of max(1, max|want|). The operands are the fixed
    draws of tests/planes_restatement.py (N(0, 1) x N(0, 0.1), and the decoder-like 0.1 x 0.05); tests/test_gemm_planes_host.py
    shows without a GPU that the modes' arithmetic alone stays under a fifth of those bounds on exactly these operands, and a
    failure message here says which of the kernel and the arithmetic moved;
  * a ReLU derivative (0 / 1) is compared where |pre-activation| exceeds the bound; where it does not, either value is right;
  * canaries: every gap column (ld > width) of every buffer and the rows after every output (to the end of a 128-row tile, and
    three more) are NaN; an input NaN that reaches a result fails the finiteness assert, and all gap columns and canary rows
    must hold the NaN bits afterwards. Inputs are allocated with exactly (rows - 1) * ld + width elements;
  * strides all differ: lda = K + 8, ldw = K + 12, ldc = N + 8, ldr = N + 16, ldp = N + 20, ldg = N + 24 (forward); ldy = C + 8,
    ldw = K + 12, ldx = K + 8, ldr = K + 16, ldm = K + 20 (input gradient); ldy = n + 8, ldx = K + 16, ldw = K + 4 (weight
    gradient). All keep the 16-byte-load condition, so a strided launch runs the same kernel in the same order as the dense
    one and must be BIT-identical to it (unsplit launches; split launches under the deterministic setting). The dense launch
    is held to float64 in the same test;
  * the tile census a case relies on is asserted from planes_restatement.tile_census (pinned to csrc/gemm_plan.h's plan_tiles
    by the host test): in the plane modes a launch is re-cut into 64 x 64 tiles when splits == 1 and 1 .. 64 tiles are left over
    a multiple of 256.

Which case reaches which epilogue of tile_epilogue (gemm_core.h). Every row below runs with 3, 2 and 1 planes (mode bf16x6 /
bf16x3 / bf16); "64" = shapes small_vec, small_scalar, one, seg and the 8 leftover tiles of mixed (64 x 64 tiles, interior
tile (0, 0) of 100 x 200), "128" = shapes big_full (every tile interior), big_ragged*, seg_big and the 256 full tiles of
mixed* (128 x 128 tiles); edge tiles of every shape take the generic loop instead of epilogue_full:
    epilogue_full<EPI_STORE>      test_forward[*-store] (64, 128); test_input_gradient[*-store]
    epilogue_full<EPI_GELU>       test_forward[*-gelu] (64, 128)
    epilogue_full<EPI_RES>        test_forward[*-res] (64, 128); test_input_gradient[*-res]
    epilogue_full<EPI_PRE_GELU>   test_forward[*-pre_gelu] (64, 128); [*-dgelu] (act_grad: stored as the pre-activation, then
                                  launch_act_grad_inplace)
    epilogue_full<EPI_ACCUM>      test_input_gradient[*-accum] (64, 128); test_weight_gradient[*] unsplit (wgrad_recut 64,
                                  wgrad_seg128 64); the tail launch of test_input_gradient_ragged_contraction
    epilogue_full<EPI_ATOMIC>     test_weight_gradient[atomics-*] split (wgrad_split4: one 128 x 128 tile, 4 splits),
                                  test_input_gradient_split_k[atomics-*] (64 x 64 output on a 128 x 128 tile: generic loop
                                  with split) - under the deterministic setting the same launches store to the workspace
    epilogue_full<EPI_RES_DROP>   test_forward[*-res_drop] (64, 128)
    generic loop (EPI_GENERIC)    test_forward[*-generic_gelu / generic_relu / generic_swish / drelu / dgelu_drop / drelu_drop /
                                  generic_drop] (64, 128), test_input_gradient[*-res_accum / mul_res]; every edge tile
    post-passes                   launch_act_grad_inplace: [*-dgelu / drelu / dgelu_drop / drelu_drop];
                                  launch_mul_inplace: test_input_gradient[*-mul / mul_res]
    workspace store (det_ws)      test_weight_gradient[ordered-*] split, test_input_gradient_split_k[ordered-*]
(EPI_ATOMIC never meets a 64 x 64 tile: a launch is re-cut only when it is unsplit.)

What these tests found. The bias gradient of the plane kernels was added into dbias by TWO atomic adds per row (the two threads
that hold a row's two k halves): an unsplit launch into a dbias that already held a contribution gave one of two results,
depending on their order - test_weight_gradient[*-accumulate] (strided against dense against a second run, bit for bit). The
kernel now adds the halves in LDS in a fixed order. vb_linear_bwd_weight zero-filled dW[0] and vb_linear_bwd_input ran its
first per-segment launch before they returned VB_E_SEGMENT for a NULL pointer in a later segment - the error-return tests
(every target untouched). Both mode-dependent refusals of the round-1 path (preact with act_grad, mul with accumulate) turned
out to hold in EVERY mode - the planners hand these combinations to the round-1 path in the f32 mode too, and no caller in
vilbert/ops.py, vilbert/autograd_ops.py or csrc/layers.hip issues them: stated in include/vilbert_hip.h and pinned here.
"""
import ctypes
import functools

import pytest
import torch

import dropout_restatement as DR
import planes_restatement as PR
from test_bf16_gemm_abi_gpu import Out, _bits, _input

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ["bf16x6", "bf16x3", "bf16", "f32"]
E_BADARG, E_ALIGN, E_RANGE, E_SEGMENT = -1, -2, -3, -4
ACT = {"none": 0, "gelu": 1, "relu": 2, "swish": 3}
MAX_SEGMENTS = 4
NAN = float("nan")
DROP_P, DROP_SEED = 0.25, 0x5EED5EED5EED
F32 = torch.float32


def _N():
    from vilbert import _native
    return _native


@pytest.fixture(params=MODES)
def mode(request):
    N = _N()
    prev = N.set_gemm_mode(request.param)
    yield request.param
    N.set_gemm_mode(prev)


@pytest.fixture(params=[True, False], ids=["ordered", "atomics"])
def det(request):
    N = _N()
    wanted = N._DET["wanted"]
    N.set_deterministic(request.param)
    yield request.param
    N.set_deterministic(wanted)


def _call(fn, args, what, expect=0):
    """One call of an entry point. The deterministic workspace is registered lazily by the Python launchers, and these tests
    call the library directly: registered here; a launch that wanted the ordered reduce and ran with atomics fails."""
    N = _N()
    N.ensure_deterministic(torch.device(DEV))
    before = N.deterministic_fallbacks()
    rc = getattr(N.lib(), fn)(N.stream_ptr(), ctypes.byref(args))
    assert rc == expect, "%s: %s returned %d, expected %d" % (what, fn, rc, expect)
    assert N.deterministic_fallbacks() == before, "%s: the ordered reduce was wanted and the launch ran with atomics" % what


_WORST, _CURRENT = {}, [""]       # (test function, mode) -> (worst error of the scale, the comparison that had it)


@pytest.fixture(autouse=True)
def _current_test(request):
    _CURRENT[0] = request.node.originalname
    yield


@pytest.fixture(autouse=True, scope="module")
def _report():
    """With -s: one line per (test function, bound) after the last test - the worst comparison it made."""
    yield
    print()
    for (test, mode), (err, what) in sorted(_WORST.items()):
        print("%-52s bound %-6s %.1e: worst %.3e of the scale (%s)" % (test, mode, PR.BOUND[mode], err, what))


def _pad(rows):
    """Canary rows after an output of `rows` rows: up to the end of a 128-row tile, and three more."""
    return (rows + 127) // 128 * 128 - rows + 3


def _close(got, want64, mode, what, pb=None):
    g = got.double()
    assert g.shape == want64.shape, what
    assert bool(torch.isfinite(g).all()), "%s: non-finite values" % what
    scale = max(1.0, float(want64.abs().max()))
    err = float((g - want64).abs().max())
    key = (_CURRENT[0], mode)
    if err / scale >= _WORST.get(key, (-1.0, ""))[0]:
        _WORST[key] = (err / scale, what)
    if err > PR.BOUND[mode] * scale:
        blame = ""
        if pb is not None:
            arith = PR.arithmetic_error(pb.a, pb.b.t().contiguous(), mode)
            blame = "; the mode's arithmetic alone errs %.3e on these operands: the %s moved" % (
                arith, "KERNEL" if arith <= PR.BOUND[mode] / 5 else "ARITHMETIC")
        raise AssertionError("%s [%s]: max err %.3e = %.3e of the scale %.3e, bound %.3e%s" % (
            what, mode, err, err / scale, scale, PR.BOUND[mode], blame))


def _same(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), "%s: the strided result differs from the dense one" % what


class Problem:
    """One problem of planes_restatement.PROBLEMS: operands a [m, k], b [n, k] on the CPU, their float64 product, and the
    epilogue operands of an [m, n] result (residual r, target contents t0, multiplier mulv = gelu' of a draw, bias)."""

    def __init__(self, name):
        self.name = name
        _fam, self.m, self.n, self.k = PR.PROBLEMS[name]
        self.a, self.b = PR.problem(name)
        seed = 100 * list(PR.PROBLEMS).index(name)
        self.acc = self.a.double() @ self.b.double().t()
        self.r = PR.rand(self.m, self.n, seed=seed + 3)
        self.t0 = PR.rand(self.m, self.n, seed=seed + 4)
        z = PR.rand(self.m, self.n, seed=seed + 5).double()
        self.mulv = (0.5 * (1 + torch.erf(z / 2 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2 * torch.pi) ** 0.5).float()
        self.bias = PR.rand(self.n, seed=seed + 6)
        self._keep = None

    def keep(self):
        """The keep mask of (DROP_P, DROP_SEED) over element index row * n + col, from the host restatement."""
        if self._keep is None:
            self._keep = torch.from_numpy(DR.keep(DROP_SEED, DR.linear_index(self.m, self.n), DROP_P))
            frac = float(self._keep.float().mean())
            assert self.m * self.n < 4096 or abs(frac - (1 - DROP_P)) < 0.05, frac
        return self._keep


@functools.lru_cache(maxsize=None)
def _problem(name):
    return Problem(name)


def _census(pb_or_shape, mode, want=None, splits=1, cseg=None):
    m, n = pb_or_shape
    got = PR.tile_census(m, n, splits, mode != "f32", cseg)
    assert want is None or got == want, "tile census of %d x %d in mode %s: %s, the case was built for %s" % (m, n, mode, got, want)
    return got


# ---------------------------------------------------------------------------------------------------------------------
# vb_linear_fwd
# ---------------------------------------------------------------------------------------------------------------------
FWD_CASES = {  # case -> (act, residual, preact, act_grad, dropout)
    "store": ("none", False, False, False, False),
    "gelu": ("gelu", False, False, False, False),
    "res": ("none", True, False, False, False),
    "pre_gelu": ("gelu", False, True, False, False),
    "generic_gelu": ("gelu", True, True, False, False),
    "generic_relu": ("relu", True, True, False, False),
    "generic_swish": ("swish", True, True, False, False),
    "dgelu": ("gelu", False, False, True, False),
    "drelu": ("relu", False, False, True, False),
    "dgelu_drop": ("gelu", True, False, True, True),
    "drelu_drop": ("relu", False, False, True, True),
    "res_drop": ("none", True, False, False, True),
    "generic_drop": ("gelu", True, True, False, True),
}


def _fwd_launch(pb, case, strided, what, nseg=1, bias=(True,), row_step=1, expect=0, ldc=None):
    """One vb_linear_fwd launch: dict of the results on the CPU (y, pre, grad), canaries checked. row_step: A is every
    row_step-th row of a taller matrix (the first-token gather of the poolers)."""
    N = _N()
    act, res, pre, grad, drop = FWD_CASES[case]
    M, Nn, K = pb.m, pb.n, pb.k
    seg_n = Nn // nseg
    assert seg_n * nseg == Nn and len(bias) == nseg
    lda = (K + 8 if strided else K) if row_step == 1 else row_step * K + 8
    ldw = K + 12 if strided else K
    if ldc is None:
        ldc = Nn + 8 if strided and not drop else Nn          # (dropout needs a contiguous C)
    ldr, ldp, ldg = (Nn + 16, Nn + 20, Nn + 24) if strided else (Nn, Nn, Nn)
    xd = _input(pb.a, lda)
    wd = [_input(pb.b[s * seg_n:(s + 1) * seg_n], ldw) for s in range(nseg)]
    bd = [pb.bias[s * seg_n:(s + 1) * seg_n].clone().to(DEV) if bias[s] else None for s in range(nseg)]
    rd = _input(pb.r, ldr) if res else None
    out = Out(M, Nn, ldc, F32, _pad(M))
    po = Out(M, Nn, ldp, F32, _pad(M)) if pre else None
    go = Out(M, Nn, ldg, F32, _pad(M)) if grad else None
    a = N.LinearArgs()
    a.M, a.K, a.nseg, a.seg_n = M, K, nseg, seg_n
    a.A, a.lda, a.ldw = xd.data_ptr(), lda, ldw
    for s in range(nseg):
        a.W[s] = wd[s].data_ptr()
        a.bias[s] = bd[s].data_ptr() if bd[s] is not None else None
    a.C, a.ldc = out.ptr, ldc
    if res:
        a.residual, a.ldr = rd.data_ptr(), ldr
    if pre:
        a.preact, a.ldp = po.ptr, ldp
    if grad:
        a.act_grad, a.ldg = go.ptr, ldg
    a.act = ACT[act]
    if drop:
        a.dropout_p, a.seed = DROP_P, DROP_SEED
    _call("vb_linear_fwd", a, what, expect)
    if expect != 0:
        for o in (out, po, go):
            if o is not None:
                o.untouched(what)
        return None
    return {"y": out.result(what), "pre": po.result(what + ", preact") if pre else None,
            "grad": go.result(what + ", act_grad") if grad else None}


def _fwd_expected(pb, case, nseg=1, bias=(True,)):
    """float64 dict (y, pre, grad, base, keep): base = what a dropped element holds (the residual or 0)."""
    act, res, _pre, _grad, drop = FWD_CASES[case]
    seg_n = pb.n // nseg
    bv = torch.cat([pb.bias[s * seg_n:(s + 1) * seg_n].double() * (1.0 if bias[s] else 0.0) for s in range(nseg)])
    pre = pb.acc + bv
    y, d = pre, None
    if act == "gelu":
        phi = 0.5 * (1 + torch.erf(pre / 2 ** 0.5))
        y, d = pre * phi, phi + pre * torch.exp(-0.5 * pre * pre) / (2 * torch.pi) ** 0.5
    elif act == "relu":
        y, d = pre.clamp(min=0), (pre > 0).double()
    elif act == "swish":
        y = pre * torch.sigmoid(pre)
    base = pb.r.double() if res else torch.zeros_like(pre)
    if drop:
        y = torch.where(pb.keep(), y * float(DR.drop_scale(DROP_P)), torch.zeros_like(y))
    return {"y": y + base, "pre": pre, "grad": d, "base": base}


def _fwd_check(pb, case, mode, what, nseg=1, bias=(True,), row_step=1):
    """Dense and strided launch of one case: both against float64, the strided results bit-identical to the dense ones."""
    act, _res, pre, grad, drop = FWD_CASES[case]
    want = _fwd_expected(pb, case, nseg, bias)
    got = {}
    for strided in (False, True):
        tag = "%s, %s" % (what, "strided" if strided else "dense")
        g = got[strided] = _fwd_launch(pb, case, strided, tag, nseg, bias, row_step)
        _close(g["y"], want["y"], mode, tag, pb)
        if pre:
            _close(g["pre"], want["pre"], mode, tag + ": preact", pb)
        if grad and act == "relu":
            # 0 / 1: compared where the pre-activation is further from 0 than its own bound
            sure = want["pre"].abs() > PR.BOUND[mode] * max(1.0, float(want["pre"].abs().max()))
            assert pb.m * pb.n < 4096 or float(sure.double().mean()) > 0.9
            assert bool(((g["grad"].double() == want["grad"]) | ~sure).all()), tag + ": relu'"
            assert bool(((g["grad"] == 0) | (g["grad"] == 1)).all()), tag + ": relu' is 0 or 1"
        elif grad:
            _close(g["grad"], want["grad"], mode, tag + ": act_grad", pb)
        if drop:
            # the mask itself: a dropped element holds exactly the residual (or 0); a kept one whose value is further
            # from that than the bound does not
            keep, base = pb.keep(), want["base"].float()
            assert bool((g["y"][~keep] == base[~keep]).all()), tag + ": a dropped element was kept"
            far = keep & ((want["y"] - want["base"]).abs() > 2 * PR.BOUND[mode] * max(1.0, float(want["y"].abs().max())))
            assert pb.m * pb.n < 4096 or float(far.double().mean()) > 0.1          # (not vacuous)
            assert bool((g["y"][far] != base[far]).all()), tag + ": a kept element was dropped"
    for key in ("y", "pre", "grad"):
        if got[True][key] is not None:
            _same(got[True][key], got[False][key], "%s: %s" % (what, key))


@pytest.mark.parametrize("case", list(FWD_CASES))
@pytest.mark.parametrize("shape", list(PR.SHAPES))
def test_forward(mode, shape, case):
    m, n, _k, planes, f32 = PR.SHAPES[shape]
    _census((m, n), mode, f32 if mode == "f32" else planes)
    _fwd_check(_problem(shape), case, mode, "fwd %s %s" % (shape, case))


def test_forward_decoder_like_operands(mode):
    _fwd_check(_problem("decoder_fwd"), "store", mode, "fwd decoder_fwd store")
    _fwd_check(_problem("decoder_fwd"), "generic_gelu", mode, "fwd decoder_fwd generic_gelu")


# 1 to 4 segments, each with its own bias (a separate allocation), one of them NULL
SEGMENT_FORMS = [(True,), (False,), (True, False), (False, True, True), (True, True, False, True)]


@pytest.mark.parametrize("case", ["store", "generic_gelu"])
@pytest.mark.parametrize("form", SEGMENT_FORMS, ids=lambda f: "".join("b" if g else "0" for g in f))
@pytest.mark.parametrize("shape,census", [("seg", (0, 8)), ("seg_big", (72, 0))])
def test_forward_segments_and_bias_forms(mode, shape, census, form, case):
    pb = _problem(shape)
    if mode != "f32":
        _census((pb.m, pb.n), mode, census)
    _fwd_check(pb, case, mode, "fwd %s %d segments %s" % (shape, len(form), case), nseg=len(form), bias=form)
    if not all(form) and len(form) > 1:
        # not vacuous: with the first given segment's bias in the NULL segment the result is outside the bound
        seg = pb.n // len(form)
        s, first = form.index(False), form.index(True)
        want = _fwd_expected(pb, "store", len(form), form)["y"][:, s * seg:(s + 1) * seg]
        wrong = want + pb.bias[first * seg:(first + 1) * seg].double()
        assert float(((wrong - want).abs() > PR.BOUND[mode] * max(1.0, float(want.abs().max()))).double().mean()) > 0.5


@pytest.mark.parametrize("shape", ["small_vec", "big_full"])
def test_forward_gathered_rows(mode, shape):
    """A = every third row of a taller matrix (lda = 3 K + 8): the first-token gather h[:, 0] of the poolers."""
    pb = _problem(shape)
    want = _fwd_expected(pb, "store")["y"]
    g = _fwd_launch(pb, "store", True, "fwd %s gathered rows" % shape, row_step=3)
    _close(g["y"], want, mode, "fwd %s gathered rows" % shape, pb)
    _same(g["y"], _fwd_launch(pb, "store", False, "fwd %s dense" % shape)["y"], "fwd %s gathered rows" % shape)


def test_forward_dropout_needs_a_contiguous_output(mode):
    pb = _problem("small_vec")
    for case in ("res_drop", "generic_drop", "drelu_drop"):
        _fwd_launch(pb, case, True, "fwd dropout with ldc != N", expect=E_ALIGN, ldc=pb.n + 8)


# ---------------------------------------------------------------------------------------------------------------------
# vb_linear_bwd_input: dX [M, K_in] (+)= (dY [M, C] . stack(W) [C, K_in] + residual) * mul, C = nseg * seg_n
# ---------------------------------------------------------------------------------------------------------------------
DGRAD_CASES = {  # case -> (accumulate, residual, mul)
    "store": (False, False, False),
    "accum": (True, False, False),
    "res": (False, True, False),
    "res_accum": (True, True, False),
    "mul": (False, False, True),
    "mul_res": (False, True, True),
}


def _dgrad_launch(pb, case, strided, what, nseg=1, expect=0):
    """One vb_linear_bwd_input launch of problem pb (a = dY [M, C], b^T = the stacked weight [C, K_in]): dX on the CPU."""
    N = _N()
    accumulate, res, mul = DGRAD_CASES[case]
    M, Kin, C = pb.m, pb.n, pb.k
    seg_n = C // nseg
    assert seg_n * nseg == C
    ldy, ldw, ldx, ldr, ldm = (C + 8, Kin + 12, Kin + 8, Kin + 16, Kin + 20) if strided else (C, Kin, Kin, Kin, Kin)
    w = pb.b.t().contiguous()
    dyd = _input(pb.a, ldy)
    wd = [_input(w[s * seg_n:(s + 1) * seg_n], ldw) for s in range(nseg)]
    rd = _input(pb.r, ldr) if res else None
    md = _input(pb.mulv, ldm) if mul else None
    out = Out(M, Kin, ldx, F32, _pad(M), init=pb.t0 if accumulate else None)
    a = N.LinearBwdInputArgs()
    a.M, a.K, a.nseg, a.seg_n = M, Kin, nseg, seg_n
    a.dY, a.ldy, a.ldw = dyd.data_ptr(), ldy, ldw
    for s in range(nseg):
        a.W[s] = wd[s].data_ptr()
    a.dX, a.ldx, a.accumulate = out.ptr, ldx, int(accumulate)
    if res:
        a.residual, a.ldr = rd.data_ptr(), ldr
    if mul:
        a.mul, a.ldm = md.data_ptr(), ldm
    _call("vb_linear_bwd_input", a, what, expect)
    if expect != 0:
        if not accumulate:
            out.untouched(what)
        return None
    return out.result(what)


def _dgrad_expected(pb, case):
    accumulate, res, mul = DGRAD_CASES[case]
    want = pb.acc + (pb.r.double() if res else 0.0)
    if mul:
        want = want * pb.mulv.double()
    return want + (pb.t0.double() if accumulate else 0.0)


def _dgrad_check(pb, case, mode, what, nseg=1, same=True):
    want = _dgrad_expected(pb, case)
    got = {}
    for strided in (False, True):
        tag = "%s, %s" % (what, "strided" if strided else "dense")
        got[strided] = _dgrad_launch(pb, case, strided, tag, nseg)
        _close(got[strided], want, mode, tag, pb)
    if same:
        _same(got[True], got[False], what)
    return got


@pytest.mark.parametrize("case", list(DGRAD_CASES))
@pytest.mark.parametrize("shape", ["small_vec", "small_scalar", "big_full", "big_ragged", "big_ragged_scalar", "one"])
def test_input_gradient(mode, shape, case):
    m, n, _k, planes, f32 = PR.SHAPES[shape]
    _census((m, n), mode, f32 if mode == "f32" else planes)
    _dgrad_check(_problem(shape), case, mode, "dgrad %s %s" % (shape, case))


@pytest.mark.parametrize("case", ["store", "mul_res"])
@pytest.mark.parametrize("shape", ["mixed", "mixed_ragged"])
def test_input_gradient_mixed_tiles(mode, shape, case):
    m, n, _k, planes, f32 = PR.SHAPES[shape]
    _census((m, n), mode, f32 if mode == "f32" else planes)
    _dgrad_check(_problem(shape), case, mode, "dgrad %s %s" % (shape, case))


@pytest.mark.parametrize("case", list(DGRAD_CASES))
def test_input_gradient_three_segments_one_launch(mode, case):
    """3 segments of 48 out-features stacked along the contraction (48 % 16 == 0: no K tile straddles two segments)."""
    _dgrad_check(_problem("dgrad_seg48"), case, mode, "dgrad 3 x 48 %s" % case, nseg=3)


@pytest.mark.parametrize("case", list(DGRAD_CASES))
def test_input_gradient_three_segments_three_launches(mode, case):
    """3 segments of 20: one launch per segment, the second and third adding into dX; residual and mul are refused."""
    pb = _problem("dgrad_seg20")
    _accumulate, res, mul = DGRAD_CASES[case]
    if res or mul:
        for strided in (False, True):
            _dgrad_launch(pb, case, strided, "dgrad 3 x 20 %s" % case, nseg=3, expect=E_SEGMENT)
    else:
        _dgrad_check(pb, case, mode, "dgrad 3 x 20 %s" % case, nseg=3)


@pytest.mark.parametrize("case", ["store", "accum"])
def test_input_gradient_ragged_contraction(mode, case):
    """264 out-features = an aligned bulk of 256 and a tail launch of 8 that adds into dX (split_ragged_k)."""
    _dgrad_check(_problem("dgrad_ragged"), case, mode, "dgrad ragged contraction %s" % case)


@pytest.mark.parametrize("case", ["store", "accum"])
@pytest.mark.parametrize("shape", ["dgrad_splitk", "dgrad_splitk_ragged"])
def test_input_gradient_split_k(mode, det, shape, case):
    """A 64 x 64 output over 4096 / 4100 out-features: the split-K route (4 splits in the plane modes by
    plan_planes_dgrad_splits; 4100 = bulk 4096 split + a tail of 4). Ordered: two runs and the strided run bit-identical;
    atomics: each within the bound."""
    pb = _problem(shape)
    assert PR.dgrad_splits(pb.m, pb.n, pb.k // 16 * 16) == 4
    got = _dgrad_check(pb, case, mode, "dgrad %s %s" % (shape, case), same=det)
    again = _dgrad_launch(pb, case, True, "dgrad %s %s, again" % (shape, case))
    _close(again, _dgrad_expected(pb, case), mode, "dgrad %s %s, again" % (shape, case), pb)
    if det:
        assert torch.equal(_bits(again), _bits(got[True])), "two ordered runs differ"


# ---------------------------------------------------------------------------------------------------------------------
# vb_linear_bwd_weight: dW[s] [seg_n, K] (+)= dY[:, s]^T . X [M, K], dbias[s] (+)= column sums of dY[:, s]
# ---------------------------------------------------------------------------------------------------------------------
def _wgrad_launch(pb, nseg, strided, accumulate, dbias, what, ldy=None, expect=0):
    """One vb_linear_bwd_weight launch of problem pb (a^T = dY [rows, nseg seg_n], b^T = X [rows, K]):
    ([dW_s], [dbias_s or None]) on the CPU, canaries checked. ldy: a given row stride of dY, allocated in full rows."""
    N = _N()
    n, K, rows = pb.m, pb.n, pb.k
    seg_n = n // nseg
    assert seg_n * nseg == n and len(dbias) == nseg
    dy, x = pb.a.t().contiguous(), pb.b.t().contiguous()
    ldx, ldw = (K + 16, K + 4) if strided else (K, K)
    if ldy is None:
        ldy = n + 8 if strided else n
        dyd = _input(dy, ldy)
    else:
        dyd = torch.full((rows, ldy), NAN)
        dyd[:, :n] = dy
        dyd = dyd.reshape(-1).to(DEV)
    xd = _input(x, ldx)
    init = accumulate
    dws = [Out(seg_n, K, ldw, F32, _pad(seg_n), init=pb.t0[s * seg_n:(s + 1) * seg_n] if init else None) for s in range(nseg)]
    dbs = [Out(1, seg_n, seg_n + 5, F32, 1, init=pb.r[s * seg_n:(s + 1) * seg_n, 0][None, :] if init else None) if dbias[s] else None
           for s in range(nseg)]
    a = N.LinearBwdWeightArgs()
    a.M, a.K, a.nseg, a.seg_n = rows, K, nseg, seg_n
    a.dY, a.ldy, a.X, a.ldx, a.ldw = dyd.data_ptr(), ldy, xd.data_ptr(), ldx, ldw
    a.accumulate = int(accumulate)
    for s in range(nseg):
        a.dW[s] = dws[s].ptr
        a.dbias[s] = dbs[s].ptr if dbs[s] is not None else None
    _call("vb_linear_bwd_weight", a, what, expect)
    return ([o.result("%s: dW %d" % (what, s)) for s, o in enumerate(dws)],
            [o.result("%s: dbias %d" % (what, s))[0] if o is not None else None for s, o in enumerate(dbs)])


def _wgrad_close(got, pb, nseg, accumulate, dbias, mode, what):
    seg_n = pb.m // nseg
    dws, dbs = got
    colsum = pb.a.double().sum(1)
    for s in range(nseg):
        sl = slice(s * seg_n, (s + 1) * seg_n)
        _close(dws[s], pb.acc[sl] + (pb.t0[sl].double() if accumulate else 0.0), mode, "%s: dW %d" % (what, s), pb)
        if dbias[s]:
            # a column sum of fp32 values in fp32: no operand is rounded, the fp32 bound holds in every mode
            _close(dbs[s], colsum[sl] + (pb.r[sl, 0].double() if accumulate else 0.0), "f32", "%s: dbias %d" % (what, s))
        else:
            assert dbs[s] is None


def _wgrad_check(pb, nseg, accumulate, dbias, mode, det, what, ldy_pad=None, split=True):
    """Dense and strided launch against float64; bit-identical to each other, and to a second run, when the launch is
    unsplit or the ordered reduce is on. ldy_pad: dY with row stride n + ldy_pad in both launches."""
    ldy = pb.m + ldy_pad if ldy_pad is not None else None
    got = {}
    for strided in (False, True):
        tag = "%s, %s" % (what, "strided" if strided else "dense")
        got[strided] = _wgrad_launch(pb, nseg, strided, accumulate, dbias, tag, ldy=ldy)
        _wgrad_close(got[strided], pb, nseg, accumulate, dbias, mode, tag)
    if det or not split:
        again = _wgrad_launch(pb, nseg, True, accumulate, dbias, what + ", again", ldy=ldy)
        names = ["dW %d" % s for s in range(nseg)] + ["dbias %d" % s for s in range(nseg)]
        for name, u, v, w in zip(names, got[True][0] + got[True][1], got[False][0] + got[False][1], again[0] + again[1]):
            if u is not None:
                _same(u, v, "%s: %s" % (what, name))
                assert torch.equal(_bits(u), _bits(w)), "%s: %s: two runs differ" % (what, name)


WGRAD_CASES = {  # case -> (problem, nseg, which segments get a bias gradient, split launch, ldy padding)
    "recut": ("wgrad_recut", 1, (True,), False, None),                     # 48 rows: unsplit, 2 tiles re-cut into 8 of 64 x 64
    "split4": ("wgrad_split4", 1, (True,), True, None),                    # 256 rows, one 128 x 128 tile, 4 splits
    "split4_nobias": ("wgrad_split4", 1, (False,), True, None),
    "ragged_rows": ("wgrad_ragged_rows", 1, (True,), True, None),          # 263 rows = bulk 256 (4 splits) + tail 7
    "seg128": ("wgrad_seg128", 3, (True, True, True), False, None),        # 3 segments of 128: one launch
    "seg128_nobias": ("wgrad_seg128", 3, (False, False, False), False, None),
    "seg128_somebias": ("wgrad_seg128", 3, (True, False, True), False, None),   # mixed dbias: one launch per segment
    "seg128_split": ("wgrad_seg128_split", 3, (True, True, True), True, None),
    "seg96": ("wgrad_seg96", 3, (True, True, True), False, None),          # 3 segments of 96: three launches
    "seg96_somebias": ("wgrad_seg96", 3, (False, True, False), False, None),
    "odd": ("wgrad_odd", 1, (True,), False, 2),                            # seg_n = 61, ldy = 63
    "pad2": ("wgrad_pad2", 1, (True,), True, 2),                           # seg_n = 122, ldy = 124: the 30522 / 30524 form
    "skinny": ("wgrad_skinny", 1, (True,), True, None),                    # K = 5, 300 rows: wgrad_skinny_kernel in every mode
}


@pytest.mark.parametrize("accumulate", [False, True], ids=["zero", "accumulate"])
@pytest.mark.parametrize("case", list(WGRAD_CASES))
def test_weight_gradient(mode, det, case, accumulate):
    name, nseg, dbias, split, ldy_pad = WGRAD_CASES[case]
    pb = _problem(name)
    if case == "recut":
        assert PR.wgrad_splits(2, 3) == 1
        _census((pb.m, pb.n), mode, (0, 8))
    if case.startswith("split4"):
        assert PR.wgrad_splits(1, 16) == 4
        _census((pb.m, pb.n), mode, (1, 0), splits=4)
    if case == "seg128":
        _census((pb.m, pb.n), mode, (0, 24), cseg=128)
    _wgrad_check(pb, nseg, accumulate, dbias, mode, det, "wgrad %s" % case, ldy_pad=ldy_pad, split=split)


def test_skinny_weight_gradient_does_not_depend_on_the_mode(det):
    """K <= 8 runs the streaming kernel, which multiplies in fp32: the same bits in every mode."""
    N = _N()
    pb = _problem("wgrad_skinny")
    got = {}
    for m in MODES:
        prev = N.set_gemm_mode(m)
        try:
            got[m] = _wgrad_launch(pb, 1, True, False, (True,), "skinny wgrad in mode %s" % m)
        finally:
            N.set_gemm_mode(prev)
        _wgrad_close(got[m], pb, 1, False, (True,), "f32", "skinny wgrad in mode %s" % m)
    if det:
        for m in MODES[:3]:
            assert torch.equal(_bits(got[m][0][0]), _bits(got["f32"][0][0])) and torch.equal(_bits(got[m][1][0]), _bits(got["f32"][1][0]))


# ---------------------------------------------------------------------------------------------------------------------
# argument checks: every return of the three entry points, in every mode
# ---------------------------------------------------------------------------------------------------------------------
def _setup(M, n, K):
    """Buffers large enough for every variation below; every output a canary."""
    z = {k: torch.zeros(v, device=DEV) for k, v in (("x", M * (K + 64)), ("w", n * (K + 64)), ("r", M * (max(n, K) + 64)),
                                                   ("dy", M * (n + 64)), ("bias", n + 64))}
    return z


def test_forward_error_returns(mode):
    N = _N()
    M, n, K = 64, 64, 32
    z = _setup(M, n, K)
    c, p, g = (Out(M, n, n + 8, F32, 4) for _ in range(3))

    def rc(null=False, **kw):
        a = N.LinearArgs()
        a.M, a.K, a.nseg, a.seg_n = M, K, 1, n
        a.A, a.lda, a.ldw = z["x"].data_ptr(), K, K
        a.W[0], a.bias[0] = z["w"].data_ptr(), z["bias"].data_ptr()
        a.C, a.ldc = c.ptr, n
        for k, v in kw.items():
            if k in ("W0", "W1"):
                a.W[int(k[1])] = v
            else:
                setattr(a, k, v)
        return N.lib().vb_linear_fwd(N.stream_ptr(), None if null else ctypes.byref(a))
    assert rc(null=True) == E_BADARG
    assert rc(A=None) == E_BADARG and rc(C=None) == E_BADARG
    for dim in ("M", "K", "seg_n"):
        assert rc(**{dim: 0}) == E_BADARG and rc(**{dim: -4}) == E_BADARG, dim
    for nseg in (0, -1, MAX_SEGMENTS + 1):
        assert rc(nseg=nseg) == E_SEGMENT, nseg
    for act in (-1, 4):
        assert rc(act=act) == E_BADARG, act
    assert rc(W0=None) == E_SEGMENT
    assert rc(nseg=2, seg_n=n // 2, W1=None) == E_SEGMENT
    for pdrop in (-0.25, 1.0, 1.5, NAN, float("inf")):
        assert rc(dropout_p=pdrop, residual=z["r"].data_ptr(), ldr=n) == E_BADARG, pdrop
    assert rc(dropout_p=0.25, ldc=n + 8) == E_ALIGN
    assert rc(dropout_p=0.25, residual=z["r"].data_ptr(), ldr=n, ldc=n + 8) == E_ALIGN
    # the pre-activation and the activation derivative in one launch: refused (include/vilbert_hip.h)
    for act in ACT.values():
        assert rc(act=act, preact=p.ptr, ldp=n, act_grad=g.ptr, ldg=n) == E_BADARG, act
    for o in (c, p, g):
        o.untouched("vb_linear_fwd error returns")
    assert rc() == 0
    torch.cuda.synchronize()


def test_input_gradient_error_returns(mode):
    N = _N()
    M, C, Kin = 64, 64, 32
    z = _setup(M, C, Kin)
    dx = Out(M, Kin, Kin + 8, F32, 4)

    def rc(null=False, **kw):
        a = N.LinearBwdInputArgs()
        a.M, a.K, a.nseg, a.seg_n = M, Kin, 1, C
        a.dY, a.ldy, a.ldw = z["dy"].data_ptr(), C, Kin
        a.W[0] = z["w"].data_ptr()
        a.dX, a.ldx = dx.ptr, Kin
        for k, v in kw.items():
            if k in ("W0", "W1", "W2"):
                a.W[int(k[1])] = v
            else:
                setattr(a, k, v)
        return N.lib().vb_linear_bwd_input(N.stream_ptr(), None if null else ctypes.byref(a))
    r = z["r"].data_ptr()
    w1 = z["w"].data_ptr() + 4 * 20 * Kin
    assert rc(null=True) == E_BADARG
    assert rc(dY=None) == E_BADARG and rc(dX=None) == E_BADARG
    for dim in ("M", "K", "seg_n"):
        assert rc(**{dim: 0}) == E_BADARG and rc(**{dim: -4}) == E_BADARG, dim
    for nseg in (0, -1, MAX_SEGMENTS + 1):
        assert rc(nseg=nseg) == E_SEGMENT, nseg
    assert rc(W0=None) == E_SEGMENT
    assert rc(nseg=2, seg_n=32, W1=None) == E_SEGMENT                               # one fused launch
    three = {"nseg": 3, "seg_n": 20, "W1": w1, "W2": w1}
    assert rc(**dict(three, W2=None)) == E_SEGMENT                                  # one launch per segment: none has run
    assert rc(residual=r, ldr=Kin, **three) == E_SEGMENT
    assert rc(mul=r, ldm=Kin, **three) == E_SEGMENT
    # a multiplier with accumulate: refused (include/vilbert_hip.h)
    assert rc(mul=r, ldm=Kin, accumulate=1) == E_BADARG
    assert rc(mul=r, ldm=Kin, residual=r, ldr=Kin, accumulate=1) == E_BADARG
    dx.untouched("vb_linear_bwd_input error returns")
    assert rc() == 0 and rc(**three) == 0
    torch.cuda.synchronize()


def test_weight_gradient_error_returns(mode):
    N = _N()
    M, n, K = 64, 64, 32
    z = _setup(M, n, K)
    dws = [Out(n, K, K + 8, F32, 4) for _ in range(2)]
    dbs = [Out(1, n, n + 8, F32, 1) for _ in range(2)]

    def rc(null=False, **kw):
        a = N.LinearBwdWeightArgs()
        a.M, a.K, a.nseg, a.seg_n = M, K, 1, n
        a.dY, a.ldy, a.X, a.ldx, a.ldw = z["dy"].data_ptr(), n, z["x"].data_ptr(), K, K
        for s in range(2):
            a.dW[s], a.dbias[s] = dws[s].ptr, dbs[s].ptr
        for k, v in kw.items():
            if k in ("dW0", "dW1"):
                a.dW[int(k[2])] = v
            else:
                setattr(a, k, v)
        return N.lib().vb_linear_bwd_weight(N.stream_ptr(), None if null else ctypes.byref(a))
    assert rc(null=True) == E_BADARG
    assert rc(dY=None) == E_BADARG and rc(X=None) == E_BADARG
    for dim in ("M", "K", "seg_n"):
        assert rc(**{dim: 0}) == E_BADARG and rc(**{dim: -4}) == E_BADARG, dim
    for nseg in (0, -1, MAX_SEGMENTS + 1):
        assert rc(nseg=nseg) == E_SEGMENT, nseg
    for accumulate in (0, 1):
        assert rc(dW0=None, accumulate=accumulate) == E_SEGMENT
        assert rc(nseg=2, seg_n=n // 2, dW1=None, accumulate=accumulate) == E_SEGMENT      # (before dW[0] is zero-filled)
    for o in dws + dbs:
        o.untouched("vb_linear_bwd_weight error returns")
    assert rc() == 0
    torch.cuda.synchronize()
