"""MX (block-scaled) e4m3 forward path (BASELINE configs[4], round 4; csrc/mx8.hip) against its CPU statement
oracle/fp8_oracle.py `mx_*` (itself pinned against torch.float8_e4m3fn in tests/test_fp8_oracle.py).

Bars (this mode's own, not the fp32 1e-4 bar - it is never the default):
  * quantiser (vb_quantize_rows_mx) and the LayerNorm that emits MX codes: codes and scale words BIT-EXACT;
  * GEMM on MX operands (vb_linear_fwd_mx): |err| <= 1e-4 sum_k |a_k w_k| against float64 sums of the dequantised operands
    (every product of two scaled e4m3 values is exact; the error is the accumulation inside the scaled MFMA), with block
    magnitudes spread over 2^-6 .. 2^6 so that a wrong K-block <-> scale assignment cannot pass (tools/mx_lab found the
    operand layout that way);
  * MX OUTPUT of a GEMM (the codes the next linear consumes): scale bytes equal to the oracle's applied to the float64
    pre-quantisation values except at binade edges (|byte difference| <= 1, rare), dequantised values within one e4m3
    rounding of them;
  * model level: drift against the real reference's golden vectors under the same bound as the row-scaled fp8 mode (0.25 of
    an output's range), every linear inside the model within 6 % relative L2 of its fp32 result on the same input.
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers
from helpers import cases
from oracle import fp8_oracle as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture
def mx_mode():
    from vilbert import _native
    prev = _native.set_gemm_mode("mxfp8")
    yield
    _native.set_gemm_mode(prev)


def _blocky(rows, K, seed, lo=-6, hi=6):
    """Random values whose magnitude changes from 32-block to 32-block (and row to row)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, K, generator=g)
    e = torch.randint(lo, hi + 1, (rows, K // 32), generator=g).float()
    return x * torch.exp2(e).repeat_interleave(32, dim=1)


def _words(m):
    return m.s.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("rows,K", [(1, 128), (7, 768), (130, 1024), (64, 3072), (33, 2048), (300, 640), (5, 4096)])
def test_mx_quantiser_is_bit_exact(rows, K):
    from vilbert import ops
    x = _blocky(rows, K, seed=rows)
    if rows > 4:
        x[3] = 0
        x[4, 32:96] = 0
    m = ops.quantize_rows_mx(x.to(DEV))
    q_ref, b_ref = F.mx_quantize(x.numpy())
    assert m.srows % 256 == 0 and m.srows >= rows
    assert np.array_equal(m.q.cpu().numpy(), q_ref), "%d codes differ" % int((m.q.cpu().numpy() != q_ref).sum())
    assert np.array_equal(F.mx_words_to_bytes(_words(m), rows), b_ref)


def test_mx_quantiser_strided_input():
    from vilbert import ops
    big = _blocky(40, 512, seed=3).to(DEV)
    view = big[:, 128:384]
    m = ops.quantize_rows_mx(view)
    q_ref, b_ref = F.mx_quantize(view.cpu().numpy())
    assert np.array_equal(m.q.cpu().numpy(), q_ref) and np.array_equal(F.mx_words_to_bytes(_words(m), 40), b_ref)


def _launch(xm, wm, M, N, K, bias=None, residual=None, act=None, out="f32"):
    from vilbert import _native as N_, ops
    a = N_.LinearMxArgs()
    a.A, a.lda, a.a_scales, a.a_srows = xm.q.data_ptr(), K, xm.s.data_ptr(), xm.srows
    a.W, a.ldw, a.w_scales, a.w_srows = wm.q.data_ptr(), K, wm.s.data_ptr(), wm.srows
    a.bias = bias.data_ptr() if bias is not None else None
    if residual is not None:
        a.residual, a.ldr = residual.data_ptr(), N
    if out == "mx":
        y = ops.MxRows(M, N, DEV, (M,))
        a.Cq, a.ldq, a.c_scales, a.c_srows = y.q.data_ptr(), N, y.s.data_ptr(), y.srows
    elif out == "bf16":
        y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        a.Cb, a.ldb16 = y.data_ptr(), N
    else:
        y = torch.full((M, N), float("nan"), device=DEV)
        a.C, a.ldc = y.data_ptr(), N
    a.M, a.N, a.K, a.act = M, N, K, N_.ACT_CODES[act]
    N_.check(N_.lib().vb_linear_fwd_mx(N_.stream_ptr(), ctypes.byref(a)), "vb_linear_fwd_mx")
    return y


SHAPES = [(256, 128, 128), (300, 768, 768), (77, 128, 256), (1, 256, 128), (640, 1024, 2048), (257, 3072, 768),
          (1000, 384, 1024), (2304, 1024, 384), (9216, 768, 768),
          # the shared tile map (csrc/persistent_map.h) beyond one tile per block: 136 tiles in 17 rows (XCD runs, row by row),
          # 160 tiles in 20 x 8 (4 x 8 patches), 264 tiles (a second round of 8)
          (4352, 1024, 128), (5120, 1024, 128), (8448, 1024, 128)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_mx_gemm_matches_oracle(M, N, K):
    from vilbert import ops
    x, w = _blocky(M, K, seed=1), _blocky(N, K, seed=2, lo=-6, hi=0)
    b = torch.randn(N, generator=torch.Generator().manual_seed(3))
    r = torch.randn(M, N, generator=torch.Generator().manual_seed(4))
    xm, wm = ops.quantize_rows_mx(x.to(DEV)), ops.quantize_rows_mx(w.to(DEV))
    y = _launch(xm, wm, M, N, K, b.to(DEV), r.to(DEV))
    da = torch.from_numpy(F.mx_dequantize(*F.mx_quantize(x.numpy()))).to(DEV)
    dw = torch.from_numpy(F.mx_dequantize(*F.mx_quantize(w.numpy()))).to(DEV)
    want = da @ dw.t() + b.to(DEV).double()[None, :] + r.to(DEV).double()      # float64 on the device (same statement)
    mag = da.abs() @ dw.abs().t() + 1.0
    err = (y.double() - want).abs()
    assert torch.isfinite(y).all()
    print("mx GEMM %dx%dx%d: max err / sum|a w| = %.2e" % (M, N, K, (err / mag).max().item()))
    assert (err <= 1e-4 * mag).all(), "max err/mag %.3e" % (err / mag).max().item()
    # bf16 output of the same values
    yb = _launch(xm, wm, M, N, K, b.to(DEV), r.to(DEV), out="bf16")
    assert (yb.double() - want).abs().le(want.abs() / 256 + 1e-4 * mag).all()


@pytest.mark.parametrize("M,N,K,act", [(256, 128, 128, "gelu"), (300, 768, 768, None), (1000, 3072, 768, "gelu"),
                                       (2304, 1024, 1024, "gelu")])
def test_mx_gemm_emits_the_codes_of_its_result(M, N, K, act):
    from vilbert import ops
    x, w = _blocky(M, K, seed=5, lo=-3, hi=3), _blocky(N, K, seed=6, lo=-6, hi=-2)
    b = torch.randn(N, generator=torch.Generator().manual_seed(7))
    xm, wm = ops.quantize_rows_mx(x.to(DEV)), ops.quantize_rows_mx(w.to(DEV))
    ym = _launch(xm, wm, M, N, K, b.to(DEV), None, act, out="mx")
    y32 = _launch(xm, wm, M, N, K, b.to(DEV), None, act, out="f32")            # the same values, unquantised (fp32 kernel output)
    # exactly the quantiser applied to the fp32 output of the same launch arithmetic
    q_ref, b_ref = F.mx_quantize(y32.cpu().numpy())
    got_b = F.mx_words_to_bytes(_words(ym), M)
    assert np.array_equal(got_b, b_ref), "%d scale bytes differ" % int((got_b != b_ref).sum())
    assert np.array_equal(ym.q.cpu().numpy(), q_ref), "%d codes differ" % int((ym.q.cpu().numpy() != q_ref).sum())
    # and against the float64 statement: within one e4m3 rounding
    want = F.linear_mx(x.numpy(), w.numpy(), b.numpy())
    if act == "gelu":
        want = F.mx_gelu(want)               # the epilogue's polynomial GELU (oracle: within 4e-4 |x| + 6e-4 of the erf form)
    back = F.mx_dequantize(ym.q.cpu().numpy(), got_b)
    scale = np.ldexp(1.0, got_b.astype(np.int32) - 127).repeat(32, axis=1)
    mag = F.mx_dequantize(*F.mx_quantize(x.numpy())).__abs__() @ np.abs(F.mx_dequantize(*F.mx_quantize(w.numpy()))).T + 1.0
    assert (np.abs(back - want) <= np.abs(want) / 16 + scale / 1024 * 1.01 + 2e-4 * mag).all()


@pytest.mark.parametrize("rows,cols,with_x2", [(37, 768, False), (130, 1024, True), (5, 2048, False)])
def test_layernorm_emits_the_same_mx_codes_as_the_quantiser(mx_mode, rows, cols, with_x2):
    from vilbert import _native, ops
    g_ = torch.Generator().manual_seed(1)
    x = (torch.randn(rows, cols, generator=g_) * 3).to(DEV)
    x2 = torch.randn(rows, cols, generator=g_).to(DEV) if with_x2 else None
    g, b = (1 + 0.1 * torch.randn(cols, generator=g_)).to(DEV), (0.1 * torch.randn(cols, generator=g_)).to(DEV)
    with torch.no_grad():
        y, _, _ = ops.layernorm_fwd(x, g, b, 1e-12, x2)
    assert hasattr(y, "_vb_mx")
    m, ver = y._vb_mx
    prev = _native.set_gemm_mode("f32")
    with torch.no_grad():
        y32, _, _ = ops.layernorm_fwd(x, g, b, 1e-12, x2)
    _native.set_gemm_mode(prev)
    assert torch.equal(y, y32) and not hasattr(y32, "_vb_mx")
    q_ref, b_ref = F.mx_quantize(y.cpu().numpy())
    assert np.array_equal(m.q.cpu().numpy(), q_ref) and np.array_equal(F.mx_words_to_bytes(_words(m), rows), b_ref)
    # the consuming linear takes the attached codes; a modified tensor (stale codes) is re-quantised
    w = (torch.randn(128, cols, generator=g_) * 0.05).to(DEV)
    with torch.no_grad():
        out_fused, _ = ops.linear_fwd(y, [w], None)
        out_sep, _ = ops.linear_fwd(y.clone(), [w], None)
        assert torch.equal(out_fused, out_sep)
        m.q.zero_()
        assert ops.linear_fwd(y, [w], None)[0].abs().max().item() == 0.0
        y.add_(1.0)
        assert ops.linear_fwd(y, [w], None)[0].abs().max().item() > 0.0
    y_grad, _, _ = ops.layernorm_fwd(x, g, b, 1e-12, x2, want_stats=True)
    assert not hasattr(y_grad, "_vb_mx")


def test_ffn_keeps_its_activation_in_mx(mx_mode, monkeypatch):
    """F.ffn in the MX mode: the up-projection returns MxRows (no fp32 tensor), the down-projection consumes it; the
    result equals the two launches chained by hand through an fp32 tensor and a quantiser pass."""
    from vilbert import functional as VF, ops
    g_ = torch.Generator().manual_seed(2)
    x = torch.randn(300, 768, generator=g_).to(DEV)
    w1, b1 = (torch.randn(3072, 768, generator=g_) * 0.03).to(DEV), torch.randn(3072, generator=g_).to(DEV)
    w2, b2 = (torch.randn(768, 3072, generator=g_) * 0.03).to(DEV), torch.randn(768, generator=g_).to(DEV)
    kinds = []
    real = ops.linear_fwd

    def spy(xin, *a, **kw):
        y, pre = real(xin, *a, **kw)
        kinds.append((type(xin).__name__, type(y).__name__))
        return y, pre

    monkeypatch.setattr(ops, "linear_fwd", spy)
    with torch.no_grad():
        y = VF.ffn(x, w1, b1, "gelu", w2, b2)
        assert kinds == [("Tensor", "MxRows"), ("MxRows", "Tensor")]
        h32, _ = real(x, [w1], [b1], "gelu")
        y_two, _ = real(h32, [w2], [b2], None, x)
    # (the MX mode keeps the residual stream in bf16: the fused call returns the same values rounded to bf16)
    assert y.dtype == torch.bfloat16 and y_two.dtype == torch.float32 and torch.equal(y, y_two.to(torch.bfloat16))
    want = torch.nn.functional.gelu(x.double() @ w1.double().t() + b1.double()) @ w2.double().t() + b2.double() + x.double()
    assert ((y.double() - want).norm() / want.norm()).item() <= 0.06


@pytest.mark.parametrize("case", ["base_2l2c_b8", "base_6l6c_b2"])
def test_mx_model_drift_is_bounded_and_reported(mx_mode, case):
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    cfg, sd, x = cases.case_inputs(case)
    m = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
    m.load_state_dict(sd)
    m = m.eval().to(DEV)
    with torch.no_grad():
        out = m(*helpers.to_device(cases.forward_args(case, x), DEV))
    gold = helpers.load_golden(case)
    worst = 0.0
    for i, n in enumerate(cases.output_names(case)):
        if n == "vision_logit":
            continue
        got = cases.sample(case, n, out[i]).cpu().double()
        want = torch.as_tensor(gold[n]).double()
        assert torch.isfinite(got).all()
        rel = ((got - want).abs().max() / want.abs().max()).item()
        worst = max(worst, rel)
        l2 = ((got - want).norm() / want.norm()).item()
        print("mxfp8 mode, %s/%s: max err %.3f of the output range, relative L2 error %.3f" % (case, n, rel, l2))
        # outputs of a handful of scalars (vil_logit: one number per sample, 8 samples) are one noise draw each: the per-layer
        # noise is the same as everywhere (3.7 % per linear, test below), measured 0.32 of the range on the 2L/2C case
        bound = 0.25 if want.numel() > 16 else 0.45
        assert rel <= bound and l2 <= bound, "%s/%s: mxfp8-mode error %.3e of the output range" % (case, n, rel)
    print("mxfp8 mode, %s: worst output error %.2e of the output range (fp32 mode: < 1e-4)" % (case, worst))
    assert worst > 1e-4


def test_mx_error_of_every_linear_inside_the_model(mx_mode, monkeypatch):
    from vilbert import _native, ops
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    case = "base_2l2c_b8"
    cfg, sd, x = cases.case_inputs(case)
    m = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
    m.load_state_dict(sd)
    m = m.eval().to(DEV)
    real = ops.linear_fwd
    seen = []

    def checked(xin, weights, biases, act=None, residual=None, **kw):
        y, pre = real(xin, weights, biases, act, residual, **kw)
        if isinstance(xin, ops.MxRows) or isinstance(y, ops.MxRows):
            # FFN pair: compare on the dequantised tensors
            xin32 = torch.from_numpy(F.mx_dequantize(xin.q.cpu().numpy(), F.mx_words_to_bytes(_words(xin), xin.rows))).float().to(DEV) \
                if isinstance(xin, ops.MxRows) else xin
            y_cmp = torch.from_numpy(F.mx_dequantize(y.q.cpu().numpy(), F.mx_words_to_bytes(_words(y), y.rows))).float().to(DEV) \
                if isinstance(y, ops.MxRows) else y
            xin32 = xin32.float() if xin32.dtype == torch.bfloat16 else xin32
            xin32 = xin32.view(-1, xin32.shape[-1])
            kw32 = {k: v for k, v in kw.items() if k != "out"}
        else:
            xin32, y_cmp, kw32 = (xin.float() if xin.dtype == torch.bfloat16 else xin), y, kw
        prev = _native.set_gemm_mode("f32")
        try:
            res32 = residual
            if res32 is not None:
                res32 = res32.float() if res32.dtype == torch.bfloat16 else res32
                if xin32 is not xin:
                    res32 = res32.view(-1, res32.shape[-1])
            y32, _ = real(xin32, weights, biases, act, res32, **kw32)
        finally:
            _native.set_gemm_mode(prev)
        w0 = weights[0] if isinstance(weights, (list, tuple)) else weights
        nseg = len(weights) if isinstance(weights, (list, tuple)) else 1
        err = ((y_cmp.double().view(-1) - y32.double().view(-1)).norm() / y32.double().norm().clamp_min(1e-30)).item()
        seen.append((y32.numel() // y32.shape[-1], nseg * w0.shape[0], w0.shape[1], act, residual is not None,
                     type(y).__name__, err))
        return y, pre

    monkeypatch.setattr(ops, "linear_fwd", checked)
    with torch.no_grad():
        m(*helpers.to_device(cases.forward_args(case, x), DEV))
    quantised = [r for r in seen if r[6] > 0.0]
    assert len(seen) >= 30 and len(quantised) >= 20, (len(seen), len(quantised))
    assert any(r[5] == "MxRows" for r in seen), "no FFN kept its activation in MX"
    worst = max(seen, key=lambda r: r[6])
    print("mxfp8 mode, per-linear relative L2 error inside %s: %d linears, %d quantised, median %.4f, worst %.4f "
          "(M=%d N=%d K=%d act=%s residual=%s out=%s)" % ((case, len(seen), len(quantised),
                                                         sorted(r[6] for r in quantised)[len(quantised) // 2], worst[6]) + worst[:6]))
    for M, Nn, K, act, res, kind, err in seen:
        assert err <= 0.06, "linear M=%d N=%d K=%d act=%s residual=%s out=%s: error %.3f of the layer's output" % (M, Nn, K, act, res, kind, err)


@pytest.mark.parametrize("B,heads,d,Sq,Sk,qb,kb", [(3, 12, 64, 36, 36, 3, 3), (2, 8, 128, 37, 37, 2, 2), (4, 8, 128, 36, 37, 4, 4),
                                                    (5, 8, 128, 9, 48, 1, 5), (2, 2, 64, 48, 17, 2, 2), (3, 8, 128, 20, 36, 3, 1)])
def test_mx_attention_matches_the_float64_statement(B, heads, d, Sq, Sk, qb, kb):
    """csrc/attention_mx.hip: bf16 q | k | v (column slices of one fused buffer), MX context. Reference: float64 softmax
    attention of the same bf16 values; the kernel rounds the probabilities to bf16 (2^-9) before P V and the result to
    e4m3 under a block scale."""
    from vilbert import ops
    H = heads * d
    g_ = torch.Generator().manual_seed(B * 100 + Sq)
    qkv_q = (torch.randn(qb, Sq, 3 * H, generator=g_) * 0.7).to(torch.bfloat16)
    qkv_k = (torch.randn(kb, Sk, 3 * H, generator=g_) * 0.7).to(torch.bfloat16)
    qkv_k[..., 2 * H:] *= torch.exp2(torch.randint(-3, 4, (kb, Sk, 1), generator=g_).float()).to(torch.bfloat16)
    keep = (torch.rand(kb, Sk, generator=g_) > 0.2).float()
    keep[:, 0] = 1
    mask = (1.0 - keep) * -10000.0
    dq, dk = qkv_q.to(DEV), qkv_k.to(DEV)
    out = ops.attention_fwd_mx(dq[..., :H], dk[..., H:2 * H], dk[..., 2 * H:], mask.to(DEV), heads)
    assert out.rows == B * Sq and out.K == H and out.lead == (B, Sq)
    q = qkv_q[..., :H].double().expand(B, Sq, H).reshape(B, Sq, heads, d).permute(0, 2, 1, 3)
    k = qkv_k[..., H:2 * H].double().expand(B, Sk, H).reshape(B, Sk, heads, d).permute(0, 2, 1, 3)
    v = qkv_k[..., 2 * H:].double().expand(B, Sk, H).reshape(B, Sk, heads, d).permute(0, 2, 1, 3)
    sc = q @ k.transpose(2, 3) / d ** 0.5 + mask.double().expand(B, Sk)[:, None, None, :]
    want = (torch.softmax(sc, dim=-1) @ v).permute(0, 2, 1, 3).reshape(B * Sq, H).numpy()
    got_b = F.mx_words_to_bytes(_words(out), B * Sq)
    got = F.mx_dequantize(out.q.cpu().numpy(), got_b)
    scale = np.ldexp(1.0, got_b.astype(np.int32) - 127).repeat(32, axis=1)
    vmax = v.abs().amax().item()
    err = np.abs(got - want)
    assert np.isfinite(got).all()
    assert (err <= np.abs(want) / 16 + scale / 1024 * 1.01 + 0.01 * vmax).all(), float((err - np.abs(want) / 16).max())
    want_b = F.mx_scale_bytes(np.abs(want.astype(np.float32)).reshape(B * Sq, H // 32, 32).max(axis=2))
    diff = np.abs(want_b.astype(np.int32) - got_b.astype(np.int32))
    assert diff.max() <= 1 and (diff > 0).mean() < 0.05, (diff.max(), (diff > 0).mean())
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("mx attention B=%d h=%d d=%d %dx%d: relative L2 error of the MX context %.4f" % (B, heads, d, Sq, Sk, rel))
    assert rel <= 0.04


def test_mx_model_uses_the_bf16_attention_and_keeps_contexts_in_mx(mx_mode, monkeypatch):
    from vilbert import ops
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    case = "base_2l2c_b8"
    cfg, sd, x = cases.case_inputs(case)
    m = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
    m.load_state_dict(sd)
    m = m.eval().to(DEV)
    calls = {"mx": 0, "f32": 0}
    real_mx, real_f32 = ops.attention_fwd_mx, ops.attention_fwd
    monkeypatch.setattr(ops, "attention_fwd_mx", lambda *a, **k: (calls.__setitem__("mx", calls["mx"] + 1), real_mx(*a, **k))[1])
    monkeypatch.setattr(ops, "attention_fwd", lambda *a, **k: (calls.__setitem__("f32", calls["f32"] + 1), real_f32(*a, **k))[1])
    with torch.no_grad():
        m(*helpers.to_device(cases.forward_args(case, x), DEV))
    # 2 text layers + 2 image layers... every self-attention and both directions of every connection layer
    assert calls["f32"] == 0 and calls["mx"] >= 6, calls


@pytest.mark.parametrize("rows,cols", [(37, 768), (130, 1024)])
def test_bf16_stream_layernorm_and_residual(mx_mode, rows, cols):
    """The bf16 residual stream of the MX mode: a GEMM adds a bf16 residual and writes the sum as bf16; the LayerNorm reads it,
    writes the next residual as bf16 and its MX codes (quantiser of the fp32 result, before the bf16 rounding)."""
    from vilbert import ops
    g_ = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, cols, generator=g_) * 2).to(torch.bfloat16).to(DEV)
    g, b = (1 + 0.1 * torch.randn(cols, generator=g_)).to(DEV), (0.1 * torch.randn(cols, generator=g_)).to(DEV)
    with torch.no_grad():
        y, _, _ = ops.layernorm_fwd(x, g, b, 1e-12)
    assert y.dtype == torch.bfloat16 and hasattr(y, "_vb_mx")
    xd = x.double()
    mu = xd.mean(1, keepdim=True)
    want = g.double() * (xd - mu) / torch.sqrt(((xd - mu) ** 2).mean(1, keepdim=True) + 1e-12) + b.double()
    assert (y.double() - want).abs().le(want.abs() / 256 + 1e-5).all()
    m = y._vb_mx[0]
    q_ref, b_ref = F.mx_quantize(want.float().cpu().numpy())
    got_b = F.mx_words_to_bytes(_words(m), rows)
    assert (np.abs(got_b.astype(np.int32) - b_ref.astype(np.int32)) <= 1).all() and (got_b != b_ref).mean() < 0.01
    back = F.mx_dequantize(m.q.cpu().numpy(), got_b)
    scale = np.ldexp(1.0, got_b.astype(np.int32) - 127).repeat(32, axis=1)
    assert (np.abs(back - want.cpu().numpy()) <= np.abs(want.cpu().numpy()) / 16 + scale / 1024 * 1.01 + 1e-5).all()
    # GEMM with a bf16 residual, bf16 sum out
    w = (torch.randn(cols, cols, generator=g_) * 0.03).to(DEV)
    bias = torch.randn(cols, generator=g_).to(DEV)
    xin = torch.randn(rows, cols, generator=g_).to(DEV)
    with torch.no_grad():
        s16, _ = ops.linear_fwd(xin, [w], [bias], None, y, out="bf16")
        s32, _ = ops.linear_fwd(xin, [w], [bias], None, y.float())
    assert s16.dtype == torch.bfloat16 and s32.dtype == torch.float32
    assert (s16.double() - s32.double()).abs().le(s32.double().abs() / 256 + 1e-6).all()


@pytest.mark.parametrize("M,N,K", [(300, 1601, 1024), (77, 3129, 2048), (40, 30522, 768)])
def test_ragged_heads_run_on_a_zero_padded_weight_copy(mx_mode, M, N, K):
    """Heads whose width is not a multiple of the GEMM's 128-column tile (1601 region classes, 3129 answers, the 30522-wide MLM
    decoder): MX GEMM on a weight copy padded with all-zero rows, result = a column slice of the padded output."""
    from vilbert import ops
    g_ = torch.Generator().manual_seed(N)
    x = torch.randn(M, K, generator=g_)
    w = torch.randn(N, K, generator=g_) * 0.05
    b = torch.randn(N, generator=g_)
    with torch.no_grad():
        y, _ = ops.linear_fwd(x.to(DEV), [w.to(DEV)], [b.to(DEV)])
    assert y.shape == (M, N) and y.stride(0) % 128 == 0 and y.stride(0) >= N
    want = F.linear_mx(x.numpy(), w.numpy(), b.numpy())
    mag = np.abs(F.mx_dequantize(*F.mx_quantize(x.numpy()))) @ np.abs(F.mx_dequantize(*F.mx_quantize(w.numpy()))).T + 1.0
    assert (np.abs(y.cpu().numpy().astype(np.float64) - want) <= 1e-4 * mag).all()
    exact = x.double() @ w.double().t() + b.double()
    assert ((y.cpu().double() - exact).norm() / exact.norm()).item() <= 0.06


@pytest.mark.parametrize("rows,K", [(7, 768), (130, 1024), (300, 640), (33, 2048)])
def test_mx_quantiser_of_bfloat16_rows_is_the_fp32_quantiser_on_the_widened_rows(rows, K):
    from vilbert import ops
    x = _blocky(rows, K, seed=rows + 1).to(torch.bfloat16)
    x[min(3, rows - 1)] = 0
    m = ops.quantize_rows_mx(x.to(DEV))
    q_ref, b_ref = F.mx_quantize(x.float().numpy())
    assert np.array_equal(m.q.cpu().numpy(), q_ref), "%d codes differ" % int((m.q.cpu().numpy() != q_ref).sum())
    assert np.array_equal(F.mx_words_to_bytes(_words(m), rows), b_ref)
    view = x.to(DEV)[:, 128:384]          # a column slice: row-strided input
    mv = ops.quantize_rows_mx(view)
    qv, bv = F.mx_quantize(x[:, 128:384].float().numpy())
    assert np.array_equal(mv.q.cpu().numpy(), qv) and np.array_equal(F.mx_words_to_bytes(_words(mv), rows), bv)


@pytest.mark.parametrize("n_tok,n_reg", [(23, 101), (20, 200)])
def test_mx_model_at_the_task_shapes_runs_its_attention_on_the_bf16_kernel(mx_mode, monkeypatch, n_tok, n_reg):
    """vilbert_tasks.yml shapes (VQA: 23 tokens x 101 regions; Visual7w: 20 x 200) in the MX inference mode: rows beyond the MX
    attention kernel's 48 go to the key-tiled bf16 kernel - never to the fp32 one - and the outputs stay within the MX mode's
    drift of the fp32 kernels (which the oracle pins at 1e-4)."""
    from oracle import synth
    from vilbert import _native, ops, ops16
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    cfg.update(v_target_size=1601)
    sd = synth.make_state_dict(cfg, "vltasks", seed=21)
    net = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=3129)
    net.load_state_dict(sd)
    net = net.eval().to(DEV)
    g = torch.Generator().manual_seed(5)
    B = 6
    ids = torch.randint(0, cfg["vocab_size"], (B, n_tok), generator=g)
    feat = torch.rand(B, n_reg, cfg["v_feature_size"], generator=g) * 2.0
    loc = torch.rand(B, n_reg, 5, generator=g)
    tmask = torch.ones(B, n_tok, dtype=torch.long)
    tmask[1, n_tok - 5:] = 0                                   # padded tokens / regions, as the task loaders produce them
    imask = torch.ones(B, n_reg, dtype=torch.long)
    imask[2, n_reg - 30:] = 0
    args = helpers.to_device((ids, feat, loc, torch.zeros(B, n_tok, dtype=torch.long), tmask, imask), DEV)
    calls = {"mx": 0, "bf16": 0, "f32": 0}
    real = {"mx": ops.attention_fwd_mx, "bf16": ops16.attention_fwd, "f32": ops.attention_fwd}
    monkeypatch.setattr(ops, "attention_fwd_mx", lambda *a, **k: (calls.__setitem__("mx", calls["mx"] + 1), real["mx"](*a, **k))[1])
    monkeypatch.setattr(ops16, "attention_fwd", lambda *a, **k: (calls.__setitem__("bf16", calls["bf16"] + 1), real["bf16"](*a, **k))[1])
    monkeypatch.setattr(ops, "attention_fwd", lambda *a, **k: (calls.__setitem__("f32", calls["f32"] + 1), real["f32"](*a, **k))[1])
    with torch.no_grad():
        got = net(*args)
    # text self-attention (23 / 20 rows): MX kernel; image self-attention and both directions of the connection layers: bf16
    assert calls["f32"] == 0 and calls["mx"] >= 2 and calls["bf16"] >= 2 + 2 * 2, calls
    prev = _native.set_gemm_mode("f32")
    try:
        with torch.no_grad():
            want = net(*args)
    finally:
        _native.set_gemm_mode(prev)
    names = ["vil_prediction", "vil_prediction_gqa", "vil_logit", "vil_binary_prediction", "vil_tri_prediction", "vision_prediction",
             "vision_logit", "linguisic_prediction", "linguisic_logit"]
    for n, a, b in zip(names, got, want):
        if not torch.is_tensor(a) or n == "vision_logit":
            continue
        a, b = a.double().cpu(), b.double().cpu()
        assert torch.isfinite(a).all(), n
        rel = ((a - b).abs().max() / b.abs().max()).item()
        l2 = ((a - b).norm() / b.norm()).item()
        print("mxfp8 mode at %d tokens x %d regions, %s: max err %.3f of the output range, relative L2 %.3f" % (n_tok, n_reg, n, rel, l2))
        bound = 0.25 if b.numel() > 16 else 0.45
        assert rel <= bound and l2 <= bound, (n, rel, l2)


@pytest.mark.parametrize("rows,cols", [(18435, 768), (16390, 1024), (20001, 256)])
def test_bf16_stream_layernorm_four_rows_per_wave_is_bit_identical(mx_mode, rows, cols):
    """Past 16,384 rows (batch 512: 18,432 token rows) the launcher gives every wave four rows instead of two, so that the
    blocks still fit the chip in one round; same arithmetic per row - y, codes and scale bytes must not change by a bit.
    Reference: the same rows through two launches of at most 16,384 rows (the two-row form)."""
    from vilbert import ops
    g_ = torch.Generator().manual_seed(rows)
    x = (torch.randn(rows, cols, generator=g_) * 2).to(torch.bfloat16).to(DEV)
    g, b = (1 + 0.1 * torch.randn(cols, generator=g_)).to(DEV), (0.1 * torch.randn(cols, generator=g_)).to(DEV)
    with torch.no_grad():
        y, _, _ = ops.layernorm_fwd(x, g, b, 1e-12)
        cut = 16384
        ya, _, _ = ops.layernorm_fwd(x[:cut].contiguous(), g, b, 1e-12)
        yb, _, _ = ops.layernorm_fwd(x[cut:].contiguous(), g, b, 1e-12)
    m, ma, mb = y._vb_mx[0], ya._vb_mx[0], yb._vb_mx[0]
    assert torch.equal(y[:cut], ya) and torch.equal(y[cut:], yb)
    assert torch.equal(m.q[:cut], ma.q) and torch.equal(m.q[cut:], mb.q)
    got = F.mx_words_to_bytes(_words(m), rows)
    assert np.array_equal(got[:cut], F.mx_words_to_bytes(_words(ma), cut))
    assert np.array_equal(got[cut:], F.mx_words_to_bytes(_words(mb), rows - cut))
