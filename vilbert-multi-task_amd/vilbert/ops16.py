"""Tensor-level launchers of the bf16 TRAINING path (csrc/gemm_bf16.hip, layernorm.hip; include/vilbert_hip.h "bf16 TRAINING
path"): the reduced-precision mode that replaces the reference's `model.half()` + apex FP16_Optimizer
(/root/reference/train_concap.py:443-461,504-505). Activations, saved tensors and activation gradients are torch.bfloat16
tensors; parameters, their gradients (the arena), LayerNorm statistics and the optimizer stay fp32. No torch arithmetic.

Weights: every launch reads a bf16 SHADOW of the (stacked) fp32 weight - row-major [N, K] for the forward, transposed
[K, N] for the input gradient (dX = dY Wt^T runs on the forward kernel) - cached per weight and refreshed when the
parameter changes (torch's version counter, or the native optimizer's `weights_changed()` epoch; refreshed IN PLACE, so
captured graphs keep their addresses).
"""
import ctypes
import os

import torch

from . import _native as N
from . import ops
from .weight_cache import DerivedWeights

BF16 = torch.bfloat16
_WEIGHTS_EPOCH = N.WEIGHTS_EPOCH


def dev_bf16(t, what):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("%s: expected a tensor on a HIP device, got %s - no CPU fallback" % (what, t.device))
    if t.dtype != BF16:
        raise RuntimeError("%s: expected bfloat16, got %s" % (what, t.dtype))
    return t.data_ptr()


def cast_bf16(x):
    """fp32 -> bfloat16 (round to nearest even), same shape."""
    x = ops._contig(x)
    y = torch.empty(x.shape, dtype=BF16, device=x.device)
    if x.numel():
        N.check(N.lib().vb_cast_f32_bf16(N.stream_ptr(), x.numel(), N.dev_f32(x, "cast input"), y.data_ptr()), "vb_cast_f32_bf16")
    return y


def cast_f32(x):
    """bfloat16 -> fp32 (exact), same shape."""
    x = ops._contig(x)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    if x.numel():
        N.check(N.lib().vb_cast_bf16_f32(N.stream_ptr(), x.numel(), dev_bf16(x, "cast input"), y.data_ptr()), "vb_cast_bf16_f32")
    return y


def eligible(K, n_out, seg_n=None, act=None):
    """Shapes the bf16 kernels serve (every linear of the two-stream encoders: 768 / 1024 / 2048 / 3072 / 4096 wide):
    forward K % 64, N % 128; input gradient N % 64, K % 128; weight gradient seg_n % 256, K % 128."""
    seg_n = n_out if seg_n is None else seg_n
    return K % 128 == 0 and n_out % 128 == 0 and seg_n % 256 == 0 and act in (None, "none", "gelu", "relu")


def _shadow_build(weights, _biases, _hint):
    """(w16 [N, K] row-major for the forward, wt16 [K, N] for the input gradient): bf16 copies of one (stacked) weight."""
    w0, nseg = weights[0], len(weights)
    seg_n, K = w0.shape
    for w in weights:
        if w.shape != (seg_n, K) or not w.is_contiguous():
            raise RuntimeError("linear (bf16): weight segments must be contiguous and equally shaped")
    if seg_n % 64 != 0 or K % 64 != 0:
        raise RuntimeError("linear (bf16): weight dimensions must be multiples of 64")
    pair = (torch.empty((nseg * seg_n, K), dtype=BF16, device=w0.device),
            torch.empty((K, nseg * seg_n), dtype=BF16, device=w0.device))
    _shadow_refresh(pair, weights, None)
    return pair


def _shadow_refresh(pair, weights, _biases):
    w16, wt16 = pair
    n, K = w16.shape
    seg_n = n // len(weights)
    for s, w in enumerate(weights):
        N.check(N.lib().vb_weight_shadow_bf16(
            N.stream_ptr(), seg_n, K, N.dev_f32(w.detach(), "linear weight"), K, w16.data_ptr() + 2 * s * seg_n * K,
            K, wt16.data_ptr() + 2 * s * seg_n, n), "vb_weight_shadow_bf16")


def _refresh_all(device):
    """ONE launch refreshes every registered shadow of `device` (the native optimizer rewrote all parameters). The table
    lives on the device and is rebuilt only when the set of registered weights changes."""
    import numpy as np
    dev_key = device.index
    t = _TABLES.get(dev_key)
    mine = _SHADOWS.entries(device)
    live = [(k, e) for k, e in mine if e.alive()]
    sig = tuple(k for k, _ in live)
    if t is None or t["sig"] != sig:
        _SHADOWS.drop([k for k, e in mine if not e.alive()])      # (weights whose model is gone)
        rec = np.dtype([("w", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("ld16", "<i8"),
                        ("ldt", "<i8"), ("tile0", "<i8")])
        rows, tile0 = [], 0
        for _k, e in live:
            w16, wt16 = e.payload
            n, K = w16.shape
            seg_n = n // len(e.wrefs)
            for s_, r in enumerate(e.wrefs):
                rows.append((r().data_ptr(), w16.data_ptr() + 2 * s_ * seg_n * K, wt16.data_ptr() + 2 * s_ * seg_n,
                             seg_n, K, K, n, tile0))
                tile0 += (seg_n // 64) * (K // 64)
        host = np.array(rows, dtype=rec)
        dev_tab = torch.from_numpy(host.view(np.uint8).reshape(-1).copy()).to(device)
        t = _TABLES[dev_key] = {"sig": sig, "tab": dev_tab, "n": len(rows), "tiles": tile0,
                                "ptrs": tuple(r[0] for r in rows)}
    elif t["ptrs"] != tuple(r().data_ptr() for _k, e in live for r in e.wrefs):
        _TABLES.pop(dev_key)                      # a parameter moved (model.to(), load into new storage): rebuild
        return _refresh_all(device)
    if t["n"]:
        N.check(N.lib().vb_weight_shadow_multi(N.stream_ptr(), t["n"], t["tab"].data_ptr(), t["tiles"]), "vb_weight_shadow_multi")
    t["epoch"] = _SHADOWS.stamp([e for _k, e in live])


# The shadows (weight_cache.py), keyed by (id(first weight tensor), number of stacked segments); a bump of the native
# optimizer's epoch refreshes ALL registered shadows of the device with one launch at the next call (an entry registered after
# the table was built, and not live in it, falls back to its own refresh). _TABLES: per device, the table of
# vb_weight_shadow_multi over every live entry (rebuilt when an entry is added or dropped) and "epoch", the
# _native.WEIGHTS_EPOCH the shadows of that device were last refreshed at by the one-launch refresh.
_SHADOWS = DerivedWeights(_shadow_build, _shadow_refresh, on_epoch=_refresh_all)
_TABLES = {}
# shadows(weights) -> (W16 [N, K] bf16, Wt16 [K, N] bf16) of the stacked segments, cached until a segment is rewritten
shadows = _SHADOWS.get


def shadow_cache_clear():
    _SHADOWS.clear()
    _TABLES.clear()
    _RAGGED.clear()


def refresh_stale(device):
    """Start of a model forward (BertModel.forward, on the stream the text / image branches fork from): when the weights
    epoch moved since the shadows of `device` were refreshed - an optimizer stepped - refresh all of them now, with the one
    launch over the device table (built here, eagerly, so that it never is built inside a stream capture or a branch)."""
    t = _TABLES.get(device.index)
    if not (t is not None and t.get("epoch") == _WEIGHTS_EPOCH[0]) and _SHADOWS.entries(device):
        with torch.no_grad():
            _refresh_all(device)
    _refresh_ragged(device)      # (the zero-padded shadows of the heads: one launch each, none when nothing is stale)


def _rows2(x, K):
    """[..., K] bf16 -> (2-D contiguous view, leading shape)."""
    x = ops._contig(x)
    return x.view(-1, K), tuple(x.shape[:-1])


def linear_fwd(x, weights, biases, act=None, residual=None, drop_p=0.0, seed=0, want_act_grad=False, out_f32=False):
    """act(x @ cat(weights).T + cat(biases)), then dropout (+ residual). x / residual bf16; returns (y, act_grad or None):
    y bf16 [..., N] (fp32 with out_f32), act_grad = gelu'(pre-activation) bf16 when asked for."""
    nseg, seg_n, K = len(weights), weights[0].shape[0], weights[0].shape[1]
    n_out = nseg * seg_n
    if x.shape[-1] != K:
        raise RuntimeError("linear: input has %d features, weight expects %d" % (x.shape[-1], K))
    w16, _ = shadows(weights)
    x2, lead = _rows2(x, K)
    M = x2.shape[0]
    y = torch.empty(lead + (n_out,), dtype=torch.float32 if out_f32 else BF16, device=x.device)
    dact = torch.empty(lead + (n_out,), dtype=BF16, device=x.device) if want_act_grad else None
    a = N.LinearBf16Args()
    a.A, a.lda, a.W, a.ldw = dev_bf16(x2, "linear input"), K, w16.data_ptr(), K
    if biases is not None:
        a.bias_segments = nseg
        for s_ in range(nseg):
            a.bias[s_] = N.dev_f32(biases[s_], "linear bias") if biases[s_] is not None else None
    if out_f32:
        a.C32, a.ldc32 = y.data_ptr(), n_out
    else:
        a.C, a.ldc = y.data_ptr(), n_out
    if residual is not None:
        residual = ops._contig(residual)
        if residual.numel() != M * n_out:
            raise RuntimeError("linear: residual shape mismatch")
        a.residual, a.ldr = dev_bf16(residual, "linear residual"), n_out
    if dact is not None:
        a.act_grad, a.ldg = dact.data_ptr(), n_out
    a.M, a.N, a.K = M, n_out, K
    a.act = N.ACT_CODES[act]
    a.dropout_p, a.seed = float(drop_p), int(seed)
    ops._timed(lambda: N.check(N.lib().vb_linear_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_linear_bf16"),
               2.0 * M * n_out * K, ("fwd16", M, seg_n, K, nseg))
    return y, dact


def linear_bwd_input(dy, weights, biases, in_features, residual=None, mul=None):
    """dX = (dY @ cat(weights)) (+ residual) (* mul): the forward kernel on the TRANSPOSED shadow. All tensors bf16."""
    nseg, seg_n = len(weights), weights[0].shape[0]
    n = nseg * seg_n
    _, wt16 = shadows(weights)
    dy2, lead = _rows2(dy, n)
    M = dy2.shape[0]
    dx = torch.empty(lead + (in_features,), dtype=BF16, device=dy.device)
    a = N.LinearBf16Args()
    a.A, a.lda, a.W, a.ldw = dev_bf16(dy2, "linear grad_output"), n, wt16.data_ptr(), n
    a.C, a.ldc = dx.data_ptr(), in_features
    if residual is not None:
        residual = ops._contig(residual)
        if residual.numel() != M * in_features:
            raise RuntimeError("linear_bwd_input: residual shape mismatch")
        a.residual, a.ldr = dev_bf16(residual, "linear residual grad"), in_features
    if mul is not None:
        mul = ops._contig(mul)
        if mul.numel() != M * in_features:
            raise RuntimeError("linear_bwd_input: multiplier shape mismatch")
        a.mul, a.ldm = dev_bf16(mul, "linear activation derivative"), in_features
    a.M, a.N, a.K = M, in_features, n
    ops._timed(lambda: N.check(N.lib().vb_linear_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_linear_bf16 (dgrad)"),
               2.0 * M * n * in_features, ("dgrad16", M, seg_n, in_features, nseg))
    return dx


def linear_bwd_weight(dy, x, nseg, seg_n, want_bias, dw_out=None, db_out=None):
    """Per segment: dW_s += dY[:, s]^T @ X (fp32, atomics into the targets) and db_s += colsum(dY[:, s]) - one launch, the
    bias gradient comes out of the fragments the weight-gradient kernel holds anyway. dy / x bf16.
    Same contract as ops.linear_bwd_weight: targets not given are slices of one zero-filled buffer allocated here.
    Deterministic setting on (default): the contraction splits go through the per-stream workspace and an ordered reduce."""
    N.ensure_deterministic(dy.device)
    n = nseg * seg_n
    dy2, _ = _rows2(dy, n)
    K = x.shape[-1]
    x2, _ = _rows2(x, K)
    M = x2.shape[0]
    if dy2.shape[0] != M:
        raise RuntimeError("linear_bwd_weight: row count mismatch")
    dws, dbs = ops.wgrad_targets(nseg, seg_n, K, want_bias, dw_out, db_out, dy.device)
    a = N.WgradBf16Args()
    a.dY, a.ldy, a.X, a.ldx = dev_bf16(dy2, "linear grad_output"), n, dev_bf16(x2, "linear input"), K
    a.M, a.K, a.nseg, a.seg_n, a.ldw = M, K, nseg, seg_n, K
    for s in range(nseg):
        a.dW[s] = N.dev_f32(dws[s], "weight gradient")
        a.dbias[s] = N.dev_f32(dbs[s], "bias gradient") if dbs[s] is not None else None
    ops._timed(lambda: N.check(N.lib().vb_wgrad_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_wgrad_bf16"),
               2.0 * M * n * K, ("wgrad16", M, seg_n, K, nseg))
    return dws, dbs


# opt-in (VB_BF16_RAGGED_WGRAD=1): measured on one box, B = 256: the decoder's weight gradient 0.326 ms on the fp32-tensor kernel
# -> 0.191 ms here + ~0.1 ms of casts, the step unchanged within 0.4 % (profiles/r06_bf16_ragged_wgrad_ab.txt)
_RAGGED_WGRAD = os.environ.get("VB_BF16_RAGGED_WGRAD", "0") == "1"


def ragged_wgrad_ok(n_out, K, rows):
    """The weight gradient of an fp32-tensor linear whose width is NOT a tile multiple (the MLM decoder: 30,522 x 768) on the
    bf16 weight-gradient kernel (linear_bwd_weight_ragged): in the bf16 mode, for outputs wide enough to pay for the two casts."""
    return _RAGGED_WGRAD and N.bf16_stream() and K % 128 == 0 and n_out >= 4096 and rows >= 64


def linear_bwd_weight_ragged(dy, x, want_bias, dw_out=None, db_out=None):
    """dW += dY^T X, db += colsum(dY) for ONE fp32-tensor linear of any output width n (round 6: the heads of the bf16 mode,
    reference vilbert.py:1178-1196 - the tied 30,522 x 768 decoder was 3.4 % (B = 256) ... 7.7 % (B = 64) of the bf16 step on
    the fp32-tensor kernel). dy fp32 [rows, n] (row-strided view allowed), x fp32 [rows, K]: both are rounded to bf16 - what
    the fp32-tensor kernel of this mode does with its operands too - dy into a buffer padded with ZERO columns to a
    multiple of 256, and vb_wgrad_bf16 writes rows < n only (n_valid). Same contract as ops.linear_bwd_weight (nseg = 1)."""
    N.ensure_deterministic(dy.device)
    n, K = dy.shape[-1], x.shape[-1]
    dy2 = dy.reshape(-1, n) if dy.dim() != 2 else dy
    x2 = ops._contig(x).reshape(-1, K)
    M = x2.shape[0]
    if dy2.shape[0] != M:
        raise RuntimeError("linear_bwd_weight: row count mismatch")
    dy16 = cast_rows_padded(dy2)
    n_pad = dy16.shape[1]
    x16 = cast_bf16(x2)
    dws, dbs = ops.wgrad_targets(1, n, K, want_bias, dw_out, db_out, dy.device)
    a = N.WgradBf16Args()
    a.dY, a.ldy, a.X, a.ldx = dy16.data_ptr(), n_pad, x16.data_ptr(), K
    a.M, a.K, a.nseg, a.seg_n, a.ldw, a.n_valid = M, K, 1, n_pad, K, n
    a.dW[0] = N.dev_f32(dws[0], "weight gradient")
    a.dbias[0] = N.dev_f32(dbs[0], "bias gradient") if dbs[0] is not None else None
    ops._timed(lambda: N.check(N.lib().vb_wgrad_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_wgrad_bf16"),
               2.0 * M * n * K, ("wgrad16", M, n, K, 1))
    # (on a weight-gradient side stream the caller has made that stream torch's current one: the two bf16 temporaries come
    # from its allocator pool)
    return dws, dbs


# ---------------------------------------------------------------------------------------------------------------
# Poolers, prediction heads and losses on the bf16 stream (csrc/heads16.hip, include/vilbert_hip_heads.h): the row kernels
# and the linear whose output width is no tile multiple (the tied 30,522-wide MLM decoder, the 1,601-wide region decoder).
# VB_BF16_HEADS=0 keeps them on the fp32-tensor kernels between two casts, as before.
# ---------------------------------------------------------------------------------------------------------------
_HEADS = {"on": os.environ.get("VB_BF16_HEADS", "1") != "0"}
# Widths from which the input gradient of a ragged linear runs in weight-gradient form (linear_ragged_bwd_input): a long
# contraction into few output tiles leaves most of the chip idle in one persistent forward-kernel launch, the weight-gradient
# kernel splits it. Below, the forward kernel on the transposed shadow. (tools/bf16_heads_bench.py times both forms.)
WGRAD_FORM_MIN_WIDTH = int(os.environ.get("VB_BF16_HEADS_WGRAD_FORM", "8192"))


def heads_enabled():
    return _HEADS["on"]


def set_heads(on):
    prev, _HEADS["on"] = _HEADS["on"], bool(on)
    return prev


def padded(n):
    """256 * ceil(n / 256) (vbh_padded)."""
    return (n + 255) // 256 * 256


def ragged_ok(K, n_out):
    """A linear of any width n_out >= 1 that the padded bf16 kernels serve (linear_ragged_*)."""
    return _HEADS["on"] and K % 128 == 0 and n_out >= 1 and n_out % 256 != 0


def _rows16(t, what):
    """(2-D row-strided bf16 view, row stride) of a [..., cols] tensor the row kernels take; copies only if it has to."""
    if not (t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.stride(0) % 8 == 0
            and t.data_ptr() % 16 == 0):
        t = ops._contig(t).view(-1, t.shape[-1])
    dev_bf16(t, what)
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


def gather_rows(src, row_map):
    """out[r] = src[row_map[r]] (bf16 [M, cols]); src bf16 [rows, cols] (row-strided view allowed), row_map int32 [M]: an entry
    outside [0, rows) (-1 = padding) gives a zero row."""
    src2, lds = _rows16(src, "gather source")
    if row_map.dtype != torch.int32 or not row_map.is_contiguous() or not row_map.is_cuda:
        raise RuntimeError("gather_rows: expected a contiguous int32 row map on a HIP device")
    M, cols = row_map.numel(), src2.shape[1]
    out = torch.empty(M, cols, dtype=BF16, device=src.device)
    N.check(N.lib().vbh_gather_rows_bf16(N.stream_ptr(), M, cols, src2.data_ptr(), lds, src2.shape[0], row_map.data_ptr(),
                                         out.data_ptr(), cols), "vbh_gather_rows_bf16")
    return out


def scatter_rows(compact, row_map, full_rows):
    """full[R] = compact[r] for the first r with row_map[r] == R, zeros elsewhere (bf16 [full_rows, cols]): the adjoint of
    gather_rows for a map that names every row once. Two launches (invert the map, write every row of `full` once)."""
    c2, ldc = _rows16(compact, "scatter source")
    M, cols = c2.shape
    if row_map.dtype != torch.int32 or not row_map.is_contiguous() or row_map.numel() != M:
        raise RuntimeError("scatter_rows: expected a contiguous int32 row map with one entry per compact row")
    inv = torch.empty(full_rows, dtype=torch.int32, device=compact.device)
    full = torch.empty(full_rows, cols, dtype=BF16, device=compact.device)
    N.check(N.lib().vbh_invert_map(N.stream_ptr(), full_rows, M, row_map.data_ptr(), inv.data_ptr()), "vbh_invert_map")
    N.check(N.lib().vbh_scatter_rows_bf16(N.stream_ptr(), full_rows, cols, c2.data_ptr(), ldc, M, inv.data_ptr(),
                                          full.data_ptr(), cols), "vbh_scatter_rows_bf16")
    return full


def relu_bwd(dy, y):
    """bf16(dy * (y > 0)) from the fp32 gradient and the fp32 OUTPUT of a ReLU (the poolers)."""
    dy, y = ops._contig(dy), ops._contig(y)
    rows, cols = ops._rows(y)
    out = torch.empty(y.shape, dtype=BF16, device=y.device)
    N.check(N.lib().vbh_relu_bwd_bf16(N.stream_ptr(), rows, cols, N.dev_f32(dy, "relu grad_output"), cols,
                                      N.dev_f32(y, "relu output"), cols, out.data_ptr(), cols), "vbh_relu_bwd_bf16")
    return out


def mul(a, b):
    """bf16(a * b) of two bf16 tensors of one shape (a gradient times the saved gelu')."""
    a, b = ops._contig(a), ops._contig(b)
    rows, cols = ops._rows(a)
    out = torch.empty_like(a)
    N.check(N.lib().vbh_mul_bf16(N.stream_ptr(), rows, cols, dev_bf16(a, "mul input"), cols, dev_bf16(b, "mul input"), cols,
                                 out.data_ptr(), cols), "vbh_mul_bf16")
    return out


def xent_bwd16(grad_loss, logits, labels, ignore_index, lse, count, want_t, want_colsum=False):
    """The cross-entropy gradient as the bf16 operands of the GEMMs in front: (G [rows, n_pad], GT [n_pad, m_pad] or None),
    pad columns / rows exact zeros. logits fp32 [rows, n] (row-strided view allowed). want_colsum: a third value, fp32
    [ceil(rows / 64), n_pad] column sums of the UNROUNDED gradient per 64 rows (colsum_parts adds them up: the bias gradient
    of the decoder in front, in fp32 as the fp32-tensor path computes it)."""
    if not ops._row_strided(logits):
        logits = ops._contig(logits)
    labels = ops._contig(labels)
    rows, n = logits.shape
    ld = logits.stride(0) if rows > 1 else max(n, logits.stride(0))
    n_pad, m_pad = padded(n), padded(rows)
    grad_loss = ops._contig(grad_loss).reshape(1)
    G = torch.empty(rows, n_pad, dtype=BF16, device=logits.device)
    GT = torch.empty(n_pad, m_pad, dtype=BF16, device=logits.device) if want_t else None
    part = torch.empty((rows + 63) // 64, n_pad, dtype=torch.float32, device=logits.device) if want_colsum else None
    N.check(N.lib().vbh_xent_bwd_bf16(
        N.stream_ptr(), rows, n, N.dev_f32(logits, "cross_entropy logits"), ld, N.dev_i64(labels, "cross_entropy labels"),
        ignore_index, N.dev_f32(lse, "cross_entropy lse"), N.dev_f32(grad_loss, "cross_entropy grad"),
        N.dev_f32(count, "cross_entropy count"), G.data_ptr(), n_pad, GT.data_ptr() if want_t else None, m_pad,
        part.data_ptr() if want_colsum else None), "vbh_xent_bwd_bf16")
    return (G, GT, part) if want_colsum else (G, GT)


def colsum_parts(part, n, out=None):
    """out[j] += sum over the rows of `part` (fp32 [parts, ld >= n]) in row order, j < n; out: fp32 [n] target (a gradient-arena
    slice) or None = a zero-filled tensor allocated here. Returns out."""
    if out is None:
        out = torch.zeros(n, dtype=torch.float32, device=part.device)
    N.check(N.lib().vbh_colsum_parts(N.stream_ptr(), part.shape[0], n, N.dev_f32(part, "column-sum partials"), part.stride(0),
                                     N.dev_f32(out, "bias gradient")), "vbh_colsum_parts")
    return out


def rows_addressable(dy2):
    """The fp32 [rows, n] tensor as the 16-byte-row addressable view the row casts take (unit column stride, row stride % 4 == 0,
    16-byte aligned); copies only if it has to."""
    n = dy2.shape[1]
    if dy2.stride(1) != 1 or dy2.stride(0) % 4 != 0 or dy2.data_ptr() % 16 != 0:
        dy2 = dy2.contiguous() if n % 4 == 0 else torch.nn.functional.pad(dy2, (0, 4 - n % 4))[:, :n]
    return dy2


def cast_rows_padded(dy2):
    """fp32 [rows, n] (any strides) -> bf16 [rows, padded(n)], pad columns zero: the padded operand of a ragged linear's
    weight-gradient and input-gradient GEMMs."""
    dy2 = rows_addressable(dy2)
    rows, n = dy2.shape
    n_pad = padded(n)
    G = torch.empty(rows, n_pad, dtype=BF16, device=dy2.device)
    N.check(N.lib().vb_cast_rows_f32_bf16(N.stream_ptr(), rows, n, N.dev_f32(dy2, "linear grad_output"), dy2.stride(0),
                                          G.data_ptr(), n_pad), "vb_cast_rows_f32_bf16")
    return G


def cast_rows_colsum(dy):
    """The fp32 gradient dy [rows, n] of a ragged decoder's logits (row stride % 4 == 0, 16-byte aligned) -> (G bf16 [rows, n_pad],
    pad columns zero; fp32 [ceil(rows / 64), n_pad] column sums of the UNROUNDED gradient per 64 rows - colsum_parts adds them up:
    the decoder's bias gradient in fp32). One pass over dy (csrc/finetune16.hip)."""
    rows, n = dy.shape
    n_pad = padded(n)
    ld = dy.stride(0) if rows > 1 else max(n, dy.stride(0))
    G = torch.empty(rows, n_pad, dtype=BF16, device=dy.device)
    part = torch.empty((rows + 63) // 64, n_pad, dtype=torch.float32, device=dy.device)
    N.check(N.lib().vbf_cast_rows_colsum(N.stream_ptr(), rows, n, N.dev_f32(dy, "linear grad_output"), ld, G.data_ptr(), n_pad,
                                         part.data_ptr()), "vbf_cast_rows_colsum")
    return G, part


def kl_bwd16(grad_loss, scores, target, lse, tsum, divisor):
    """The KL gradient as bf16 G [rows, n_pad] (pad columns zero); scores fp32 [rows, n] (row-strided view allowed)."""
    if not ops._row_strided(scores):
        scores = ops._contig(scores)
    target = ops._contig(target)
    rows, n = scores.shape
    ld = scores.stride(0) if rows > 1 else max(n, scores.stride(0))
    n_pad = padded(n)
    grad_loss = ops._contig(grad_loss).reshape(1)
    G = torch.empty(rows, n_pad, dtype=BF16, device=scores.device)
    dh, dd, _keep = ops._divisor(divisor)
    N.check(N.lib().vbh_kl_bwd_bf16(
        N.stream_ptr(), rows, n, N.dev_f32(scores, "kl_div scores"), ld, N.dev_f32(target, "kl_div target"), n,
        N.dev_f32(lse, "kl_div lse"), N.dev_f32(tsum, "kl_div tsum"), N.dev_f32(grad_loss, "kl_div grad"), dh, dd,
        G.data_ptr(), n_pad), "vbh_kl_bwd_bf16")
    return G


def _ragged_build(weights, biases, _hint):
    """{w16 [n_pad, K], wt16 [K, n_pad], bias [n_pad] fp32}: the zero-padded bf16 shadow of ONE fp32 weight [n, K] and bias."""
    w = weights[0]
    n, K = w.shape
    if len(weights) != 1 or not w.is_contiguous() or K % 64 != 0:
        raise RuntimeError("linear (bf16, ragged width): one contiguous weight with K % 64 == 0 expected")
    n_pad = padded(n)
    pay = {"w16": torch.empty(n_pad, K, dtype=BF16, device=w.device), "wt16": torch.empty(K, n_pad, dtype=BF16, device=w.device),
           "bias": torch.empty(n_pad, dtype=torch.float32, device=w.device), "bref": None}
    _ragged_refresh(pay, weights, biases)
    return pay


def _ragged_refresh(pay, weights, biases):
    import weakref
    w = weights[0]
    b = biases[0] if biases else None
    n, K = w.shape
    pay["bref"] = weakref.ref(b) if b is not None else None
    N.check(N.lib().vbh_weight_shadow_ragged(
        N.stream_ptr(), n, K, N.dev_f32(w.detach(), "linear weight"), K,
        N.dev_f32(ops._contig(b.detach()), "linear bias") if b is not None else None, pay["w16"].data_ptr(),
        pay["wt16"].data_ptr(), pay["bias"].data_ptr()), "vbh_weight_shadow_ragged")


# the padded shadows: keyed like _SHADOWS; vb_weight_shadow_multi walks whole 64-row tiles of its sources, so these are not in
# its table - refresh_stale() refreshes each stale one with its own launch
_RAGGED = DerivedWeights(_ragged_build, _ragged_refresh, bias_versions=True)


def ragged_shadows(weight, bias):
    return _RAGGED.get([weight], [bias])


def _refresh_ragged(device):
    epoch = _WEIGHTS_EPOCH[0]
    for _k, e in _RAGGED.entries(device):
        if e.epoch == epoch or not e.alive():
            continue
        w = e.wrefs[0]()
        bref = e.payload["bref"]
        b = bref() if bref is not None else None
        if bref is not None and b is None:
            continue
        with torch.no_grad():
            _ragged_refresh(e.payload, [w], [b])
        e.vers, e.epoch = _RAGGED._versions([w], [b]), epoch


def linear_ragged_fwd(x, weight, bias):
    """x @ weight.T + bias for a weight [n, K] of any height n: vb_linear_bf16 on the zero-padded shadow, fp32 result in a
    [rows, n_pad] buffer; returns its [..., n] view (row stride n_pad: 16-byte aligned rows for the loss kernels)."""
    n, K = weight.shape
    pay = ragged_shadows(weight, bias)
    n_pad = pay["w16"].shape[0]
    x2, lead = _rows2(x, K)
    M = x2.shape[0]
    y = torch.empty(M, n_pad, dtype=torch.float32, device=x.device)
    a = N.LinearBf16Args()
    a.A, a.lda, a.W, a.ldw = dev_bf16(x2, "linear input"), K, pay["w16"].data_ptr(), K
    if bias is not None:
        a.bias[0] = pay["bias"].data_ptr()
    a.C32, a.ldc32 = y.data_ptr(), n_pad
    a.M, a.N, a.K = M, n_pad, K
    if M:
        ops._timed(lambda: N.check(N.lib().vb_linear_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_linear_bf16 (ragged)"),
                   2.0 * M * n_pad * K, ("fwd16", M, n_pad, K, 1))
    y = y[:, :n]
    return y if len(lead) == 1 else y.reshape(lead + (n,))


def linear_ragged_bwd_input(G, GT, weight, bias, rows, form=None):
    """dX bf16 [rows, K] = G[:, :n] @ weight from the padded bf16 gradient G [rows, n_pad] (GT [n_pad, m_pad] = its transpose,
    or None). form "dgrad": the forward kernel on the transposed padded shadow. form "wgrad" (needs GT): the weight-gradient
    kernel, dX = GT^T w16 accumulated in fp32 into a zero-filled buffer - its contraction splits and, in the deterministic
    setting, the ordered reduce come from the planner - then one cast. Default: "wgrad" from WGRAD_FORM_MIN_WIDTH columns."""
    n, K = weight.shape
    pay = ragged_shadows(weight, bias)
    n_pad = pay["w16"].shape[0]
    if form is None:
        form = "wgrad" if GT is not None and n_pad >= WGRAD_FORM_MIN_WIDTH else "dgrad"
    if form == "wgrad":
        N.ensure_deterministic(G.device)
        m_pad = GT.shape[1]
        dx32 = torch.zeros(rows, K, dtype=torch.float32, device=G.device)
        a = N.WgradBf16Args()
        a.dY, a.ldy, a.X, a.ldx = dev_bf16(GT, "linear grad_output (transposed)"), m_pad, pay["w16"].data_ptr(), K
        a.M, a.K, a.nseg, a.seg_n, a.ldw, a.n_valid = n_pad, K, 1, m_pad, K, rows
        a.dW[0] = dx32.data_ptr()
        ops._timed(lambda: N.check(N.lib().vb_wgrad_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_wgrad_bf16 (input gradient)"),
                   2.0 * rows * n_pad * K, ("dgrad16w", rows, n_pad, K, 1))
        return cast_bf16(dx32)
    dx = torch.empty(rows, K, dtype=BF16, device=G.device)
    a = N.LinearBf16Args()
    a.A, a.lda, a.W, a.ldw = dev_bf16(G, "linear grad_output"), n_pad, pay["wt16"].data_ptr(), n_pad
    a.C, a.ldc = dx.data_ptr(), K
    a.M, a.N, a.K = rows, K, n_pad
    ops._timed(lambda: N.check(N.lib().vb_linear_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_linear_bf16 (dgrad, ragged)"),
               2.0 * rows * n_pad * K, ("dgrad16", rows, n_pad, K, 1))
    return dx


def linear_ragged_bwd_weight(G, x, n, want_bias, dw_out=None, db_out=None):
    """dW [n, K] += G[:, :n]^T x, db [n] += colsum(G[:, :n]) straight from the padded bf16 gradient G [rows, n_pad]: one
    vb_wgrad_bf16 launch that writes rows < n only. Same contract as linear_bwd_weight (nseg = 1)."""
    N.ensure_deterministic(G.device)
    K = x.shape[-1]
    x2, _ = _rows2(x, K)
    M, n_pad = G.shape
    if x2.shape[0] != M:
        raise RuntimeError("linear_bwd_weight: row count mismatch")
    dws, dbs = ops.wgrad_targets(1, n, K, want_bias, dw_out, db_out, G.device)
    a = N.WgradBf16Args()
    a.dY, a.ldy, a.X, a.ldx = dev_bf16(G, "linear grad_output"), n_pad, dev_bf16(x2, "linear input"), K
    a.M, a.K, a.nseg, a.seg_n, a.ldw, a.n_valid = M, K, 1, n_pad, K, n
    a.dW[0] = N.dev_f32(dws[0], "weight gradient")
    a.dbias[0] = N.dev_f32(dbs[0], "bias gradient") if dbs[0] is not None else None
    ops._timed(lambda: N.check(N.lib().vb_wgrad_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_wgrad_bf16 (ragged)"),
               2.0 * M * n * K, ("wgrad16", M, n, K, 1))
    return dws, dbs


# ---------------------------------------------------------------------------------------------------------------
# The skinny-output linear of the fine-tuning heads (csrc/finetune16.hip, include/vilbert_hip_finetune.h): 1 .. 4 outputs per
# bf16 row (`vision_logit`, `linguisic_logit` of VILBertForVLTasks), the input dropout drawn inside the kernels, the fp32
# master weight read as it is (no shadow).
# ---------------------------------------------------------------------------------------------------------------
SKINNY_MAX_N, SKINNY_MAX_K = 4, 2048      # VBF_MAX_N, VBF_MAX_K


def skinny_ok(K, n):
    """Shapes the skinny-output kernels serve."""
    return 1 <= n <= SKINNY_MAX_N and 8 <= K <= SKINNY_MAX_K and K % 8 == 0


def _skinny_weight(weight):
    w = weight.detach()
    if w.dim() != 2 or not w.is_contiguous() or not skinny_ok(w.shape[1], w.shape[0]):
        raise RuntimeError("skinny linear: a contiguous weight [n <= %d, K <= %d, K %% 8 == 0] expected, got %s"
                           % (SKINNY_MAX_N, SKINNY_MAX_K, tuple(weight.shape)))
    return w, w.shape[0], w.shape[1]


def _rows32(t, n, what):
    """(2-D row-strided fp32 view [rows, n], row stride) of a [..., n] tensor; copies only if it has to."""
    if not (ops._row_strided(t) and t.data_ptr() % 16 == 0):
        t = ops._contig(t).view(-1, n)
    N.dev_f32(t, what)
    return t, (t.stride(0) if t.shape[0] > 1 else max(n, t.stride(0)))


def skinny_fwd(x, weight, bias=None, row_add=None, drop_p=0.0, seed=0, out=None):
    """dropout(x, drop_p) @ weight.T + bias + row_add[:, None] -> fp32 [..., n]. x bf16 [..., K] (a 2-D row-strided view is read
    in place), weight fp32 [n, K], bias fp32 [n] or None, row_add fp32 with one value per row or None. The mask is that of
    vb_dropout over the dense [rows, K] tensor. out: a 2-D fp32 [rows, n] target (row stride >= n) or None."""
    w, n, K = _skinny_weight(weight)
    if x.shape[-1] != K:
        raise RuntimeError("skinny linear: input has %d features, weight expects %d" % (x.shape[-1], K))
    lead = tuple(x.shape[:-1])
    x2, ldx = _rows16(x, "skinny linear input")
    rows = x2.shape[0]
    if out is None:
        out = torch.empty(lead + (n,), dtype=torch.float32, device=x.device)
        o2, ldo = out.view(-1, n), n
    else:
        if out.shape != (rows, n) or not ops._row_strided(out):
            raise RuntimeError("skinny linear: out must be a row-strided [rows, n] tensor")
        o2, ldo = out, (out.stride(0) if rows > 1 else max(n, out.stride(0)))
    if row_add is not None:
        row_add = ops._contig(row_add)
        if row_add.numel() != rows:
            raise RuntimeError("skinny linear: row_add needs one value per row")
    N.check(N.lib().vbf_skinny_linear_fwd(
        N.stream_ptr(), rows, K, n, x2.data_ptr(), ldx, N.dev_f32(w, "skinny linear weight"), K,
        N.dev_f32(ops._contig(bias.detach()), "skinny linear bias") if bias is not None else None,
        N.dev_f32(row_add, "skinny linear row_add"), N.dev_f32(o2, "skinny linear output"), ldo, float(drop_p), int(seed)),
        "vbf_skinny_linear_fwd")
    return out


def skinny_bwd_input(dy, weight, drop_p=0.0, seed=0, out=None):
    """dX bf16 [..., K] = dropout-mask * scale * (dY @ weight); dy fp32 [..., n]. out: a 2-D bf16 [rows, K] target (row stride
    >= K, a multiple of 8) or None."""
    w, n, K = _skinny_weight(weight)
    lead = tuple(dy.shape[:-1])
    dy2, ldy = _rows32(dy, n, "skinny linear grad_output")
    rows = dy2.shape[0]
    if out is None:
        out = torch.empty(lead + (K,), dtype=BF16, device=dy.device)
        d2, ldd = out.view(-1, K), K
    else:
        if out.shape != (rows, K) or not ops._row_strided(out):
            raise RuntimeError("skinny linear: out must be a row-strided [rows, K] tensor")
        d2, ldd = out, (out.stride(0) if rows > 1 else max(K, out.stride(0)))
    N.check(N.lib().vbf_skinny_linear_bwd_input(
        N.stream_ptr(), rows, K, n, dy2.data_ptr(), ldy, N.dev_f32(w, "skinny linear weight"), K, dev_bf16(d2, "skinny linear dx"),
        ldd, float(drop_p), int(seed)), "vbf_skinny_linear_bwd_input")
    return out


_SKINNY_WS = {}


def skinny_bwd_weight(dy, x, n, want_bias, dw_out=None, db_out=None, drop_p=0.0, seed=0):
    """dW [n, K] += dY^T dropout(x), db [n] += colsum(dY): ADDED into the targets, as linear_bwd_weight does (nseg = 1; targets
    not given are zero-filled here). dy fp32 [..., n], x bf16 [..., K]. Two launches through a per-(device, stream) workspace
    (grow-only, like the LayerNorm backward's), bit-identical from run to run. Returns ([dW], [db or None])."""
    K = x.shape[-1]
    if not skinny_ok(K, n):
        raise RuntimeError("skinny linear: shape (K = %d, n = %d) is not served" % (K, n))
    x2, ldx = _rows16(x, "skinny linear input")
    dy2, ldy = _rows32(dy, n, "skinny linear grad_output")
    rows = x2.shape[0]
    if dy2.shape[0] != rows:
        raise RuntimeError("skinny linear: row count mismatch")
    dws, dbs = ops.wgrad_targets(1, n, K, [bool(want_bias)], [dw_out] if dw_out is not None else None,
                                 [db_out] if db_out is not None else None, x.device)
    floats = N.lib().vbf_skinny_wgrad_workspace(rows, K, n)
    key = (x.device.index, N.raw_stream(x.device.index))
    ws = _SKINNY_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = _SKINNY_WS[key] = torch.empty(max(floats, 1 << 20), dtype=torch.float32, device=x.device)
    N.check(N.lib().vbf_skinny_linear_bwd_weight(
        N.stream_ptr(), rows, K, n, dy2.data_ptr(), ldy, x2.data_ptr(), ldx, N.dev_f32(dws[0], "weight gradient"), K,
        N.dev_f32(dbs[0], "bias gradient") if dbs[0] is not None else None, ws.data_ptr(), float(drop_p), int(seed)),
        "vbf_skinny_linear_bwd_weight")
    return dws, dbs


def layernorm_fwd(x, gamma, beta, eps, want_stats=False):
    x = ops._contig(x)
    rows, cols = ops._rows(x)
    y = torch.empty_like(x)
    mean = rstd = None
    if want_stats:
        mean = torch.empty(rows, dtype=torch.float32, device=x.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    N.check(N.lib().vb_layernorm_fwd_bf16(
        N.stream_ptr(), rows, cols, dev_bf16(x, "layernorm input"), N.dev_f32(gamma, "layernorm weight"),
        N.dev_f32(beta, "layernorm bias"), eps, y.data_ptr(), mean.data_ptr() if want_stats else None,
        rstd.data_ptr() if want_stats else None), "vb_layernorm_fwd_bf16")
    return y, mean, rstd


_LN_WS = {}


def _ln_workspace(device, floats):
    """Partial dgamma / dbeta rows of one LayerNorm backward: one grow-only buffer per (device, stream) - the two kernels of a
    launch pair are ordered on their stream, and streams that run concurrently get their own."""
    key = (device.index, N.raw_stream(device.index))
    ws = _LN_WS.get(key)
    if ws is None or ws.numel() < floats:
        ws = _LN_WS[key] = torch.empty(max(floats, 1 << 20), dtype=torch.float32, device=device)
    return ws


def layernorm_bwd(dy, x, mean, rstd, gamma, dgamma=None, dbeta=None, drop=None):
    """(dx, dgamma, dbeta[, dx under the dropout mask `drop` = (p, seed) of the dense layer in front]); dy / x / dx bf16,
    dgamma / dbeta fp32 [cols] targets (OVERWRITTEN)."""
    dy, x = ops._contig(dy), ops._contig(x)
    rows, cols = ops._rows(x)
    dx = torch.empty_like(x)
    dgamma = dgamma if dgamma is not None else torch.empty(cols, dtype=torch.float32, device=x.device)
    dbeta = dbeta if dbeta is not None else torch.empty(cols, dtype=torch.float32, device=x.device)
    ws = _ln_workspace(x.device, (rows + 15) // 16 * 2 * cols)      # = vb_layernorm_bwd_bf16_workspace(rows, cols)
    twin = drop is not None and drop[0] > 0.0
    dxd = torch.empty_like(x) if twin else None
    N.check(N.lib().vb_layernorm_bwd_bf16(
        N.stream_ptr(), rows, cols, dev_bf16(dy, "layernorm grad_output"), dev_bf16(x, "layernorm input"),
        N.dev_f32(mean, "layernorm mean"), N.dev_f32(rstd, "layernorm rstd"), N.dev_f32(gamma, "layernorm weight"),
        dx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), dxd.data_ptr() if twin else None,
        float(drop[0]) if twin else 0.0, int(drop[1]) if twin else 0), "vb_layernorm_bwd_bf16")
    return (dx, dgamma, dbeta, dxd) if twin else (dx, dgamma, dbeta)


def dropout(x, p, seed):
    """dropout of a bf16 tensor (rare path: the LayerNorm backward normally hands over the masked gradient): through the fp32
    kernel and two casts."""
    return cast_bf16(ops.dropout(cast_f32(x), p, seed))


def attention_fwd(q, k, v, mask_add, heads, want_lse=False, drop_p=0.0, seed=0):
    """bf16 q [Bq, Sq, H*], k / v [Bk, Sk, H*] row-strided views (column slices of the fused projection); fp32 additive mask.
    Returns (ctx bf16 [B, Sq, H], lse fp32 [B, heads, Sq] or None). At most ops.MAX_KEYS keys."""
    if k.shape[1] > ops.MAX_KEYS:
        raise RuntimeError("attention (bf16): %d keys - one launch serves at most %d" % (k.shape[1], ops.MAX_KEYS))
    a, keep, (B, Sq, Sk, H) = ops._attn_args(q, k, v, mask_add, heads, drop_p, seed, dev_bf16)
    out = torch.empty(B, Sq, H, dtype=BF16, device=q.device)
    lse = torch.empty(B, heads, Sq, dtype=torch.float32, device=q.device) if want_lse else None
    a.O, a.ldo = out.data_ptr(), H
    a.lse = lse.data_ptr() if want_lse else None
    N.check(N.lib().vb_attention_fwd_bf16(N.stream_ptr(), ctypes.byref(a)), "vb_attention_fwd_bf16")
    return out, lse


def attention_bwd(d_out, q, k, v, mask_add, heads, lse, dq, dk, dv, drop_p=0.0, seed=0):
    """Writes dq / dk / dv (bf16 row-strided views, e.g. column slices of one fused gradient buffer) in place."""
    a, keep, (B, Sq, Sk, H) = ops._attn_args(q, k, v, mask_add, heads, drop_p, seed, dev_bf16)
    d_out = ops._contig(d_out)
    a.lse = N.dev_f32(lse, "attention lse")
    g = N.AttentionGrads()
    g.dO, g.lddo = dev_bf16(d_out, "attention grad_output"), H
    g.dQ, g.lddq = dev_bf16(dq, "attention dq"), dq.stride(1)
    g.dK, g.lddk = dev_bf16(dk, "attention dk"), dk.stride(1)
    g.dV, g.lddv = dev_bf16(dv, "attention dv"), dv.stride(1)
    dvec = torch.empty(B, heads, Sq, dtype=torch.float32, device=q.device)
    g.dvec = dvec.data_ptr()
    N.check(N.lib().vb_attention_bwd_bf16(N.stream_ptr(), ctypes.byref(a), ctypes.byref(g)), "vb_attention_bwd_bf16")
