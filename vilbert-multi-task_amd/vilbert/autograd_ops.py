"""``torch.autograd.Function`` wrappers: forward AND backward run only kernels of libvilbert_hip.so.

What torch autograd contributes is the graph bookkeeping (and the few gradient additions where a
tensor feeds two consumers); every gradient *computation* below is a native kernel:
dgrad / wgrad MFMA GEMMs (bias gradient fused into wgrad), GELU / ReLU backward, LayerNorm backward
(deterministic two-stage column reduction), the two-pass attention backward, embedding scatter-add
and the counter-based dropout mask that forward and backward regenerate from (seed, index).
"""
import itertools

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _native as N
from . import arena as _arena
from . import ops
from . import ops16

BF16 = torch.bfloat16

_seed_counter = itertools.count(1)


def next_seed():
    """64-bit dropout seed: torch's initial seed (so torch.manual_seed makes runs repeatable) mixed
    with a per-process call counter. No device sync."""
    return ((torch.initial_seed() & 0xFFFFFFFF) * 0x9E3779B1 + next(_seed_counter) * 0x632BE59BD9B4E019) \
        & 0xFFFFFFFFFFFFFFFF


# bf16 TRAINING path (round 5; ops16.py, csrc/gemm_bf16.hip): the nodes below serve both streams - on bfloat16 activations they
# launch the ops16 kernels, otherwise the ops ones. Parameters, their gradients (arena slices, fp32), LayerNorm statistics and
# the softmax statistics stay fp32. What the reference does with `model.half()` + apex FP16_Optimizer
# (train_concap.py:443-461,504-505), without loss scaling (bf16 keeps fp32's exponent range).
def _ops(t):
    """Launcher module of t's stream. Callers look the launcher up on it at call time, never bind it at import."""
    return ops16 if t.dtype == BF16 else ops


# the two launchers whose bf16 form takes other arguments: ops16.linear_bwd_input has a (unused) biases slot,
# ops16.attention_fwd has no probabilities tensor
def _dgrad(dy, weights, in_features, residual=None, mul=None):
    if dy.dtype == BF16:
        return ops16.linear_bwd_input(dy, weights, None, in_features, residual, mul)
    return ops.linear_bwd_input(dy, weights, in_features, residual, mul)


def attention_fwd(q, k, v, mask_add, heads, want_probs, want_lse, drop_p, seed):
    """ops.attention_fwd's contract on either stream: (ctx, probs or None, lse or None); bf16 has no probabilities."""
    if q.dtype == BF16:
        out, lse = ops16.attention_fwd(q, k, v, mask_add, heads, want_lse, drop_p, seed)
        return out, None, lse
    return ops.attention_fwd(q, k, v, mask_add, heads, want_probs, want_lse, drop_p, seed)


# ---------------------------------------------------------------------------------------------------------------
# Weight-gradient side streams. dW / db are not on the critical path of backward (only the optimizer / the gradient
# all-reduce read them), so every wgrad GEMM whose targets are FRESH gradient-arena slices is enqueued on a side stream
# of the stream its backward node runs on: the GPU then always holds a second, independent GEMM whose blocks fill the
# tail / prologue / epilogue bubbles of the dgrad chain (tools/gemm_lab LAB_STREAMS=1: a dgrad + wgrad pair runs
# 6-12 % faster on two streams than back to back on one). Rules that keep it race-free:
#   * only "fresh" claims go to the side stream; a second writer of a slice ("accum": tied weights, gradient
#     accumulation) first joins the side streams and then runs in order;
#   * the side streams are joined into the calling stream at the end of the backward pass (arena end-pass hook) and
#     before a data-parallel bucket is all-reduced (distributed.py);
#   * dy / x are record_stream()ed on the side stream (autograd may free them as soon as the node returns).
# VB_WGRAD_STREAM=0 disables it.
# ---------------------------------------------------------------------------------------------------------------
import collections as _collections
import os as _os

_WGRAD = {"on": _os.environ.get("VB_WGRAD_STREAM", "1") != "0", "streams": {}, "used": {}, "held": {}}


def set_wgrad_stream(on):
    prev, _WGRAD["on"] = _WGRAD["on"], bool(on)
    return prev


def _wgrad_stream(device, raw):
    """(side stream, torch.cuda.Stream object of the raw stream `raw`) for weight gradients of work launched on `raw`.
    Keyed on the raw handle so that the hot path never builds Stream objects (tools/host_profile.py); `raw` must be
    the stream that is current on `device` when this is called."""
    key = (device.index, raw)
    ent = _WGRAD["streams"].get(key)
    if ent is None:
        ent = _WGRAD["streams"][key] = (torch.cuda.Stream(device=device), torch.cuda.current_stream(device))
    return ent


def join_wgrad_streams(into=None, clear=False):
    """Make `into` (default: the current stream) wait for every weight-gradient side stream of ITS device with work in
    flight (the bookkeeping is per device: backward threads of different devices never touch each other's entry)."""
    used = _WGRAD["used"]
    if not used:
        return
    mine = used.get(into.device.index if into is not None else N.current_device())
    if not mine:
        return
    cur = into if into is not None else torch.cuda.current_stream()
    for st in list(mine.values()):
        cur.wait_stream(st)
    if clear:
        mine.clear()
        for q in _WGRAD["held"].values():
            q.clear()


def hold_for_side_stream(ws, *tensors):
    """A gradient tensor that a weight-gradient launch on side stream `ws` still READS and that the same backward node hands
    back to autograd (the skip-connection gradient passing through a dense + residual node) must not be updated in place
    while that launch is pending - and autograd's input buffers do exactly that (`old += new`) when they hold the only
    reference to the first arrival. The stream order of the in-place add covers the node's own stream, not its side
    stream (seen as a rare wrong dW with two processes time-slicing one GPU: tests/test_ddp_two_ranks_one_gpu.py, round
    6). A second reference, kept until the launch has finished (event on `ws`; under stream capture: until the end of the
    pass), sends the engine down its out-of-place path."""
    q = _WGRAD["held"].get(ws.cuda_stream)
    if q is None:
        q = _WGRAD["held"][ws.cuda_stream] = _collections.deque()
    if torch.cuda.is_current_stream_capturing():
        q.append((None, tensors))
        return
    ev = torch.cuda.Event()
    ev.record(ws)
    q.append((ev, tensors))
    while q and q[0][0] is not None and q[0][0].query():
        q.popleft()


_arena.END_PASS_HOOKS.append(lambda: join_wgrad_streams(clear=True))


class _Claims(object):
    """Gradient targets of a group of parameters for one backward node: gradient-arena slices where the arena
    manages the parameter (the kernels add in place, autograd gets an alias or None - see arena.py), else None
    (the launcher allocates)."""

    def __init__(self, params, needed):
        self.c = [(_arena.claim(p) if (n and p is not None) else (None, None, None, None)) for p, n in zip(params, needed)]
        if any(c[1] == "accum" for c in self.c):
            join_wgrad_streams()          # the earlier writer of that slice may still be running on a side stream

    def views(self):
        return [c[0] for c in self.c]

    def out(self, i, fallback):
        _view, mode, ar, idx = self.c[i]
        return _arena.result(mode, ar, idx, fallback)

    def fresh_or_none(self, i):
        """target for a kernel that OVERWRITES (LayerNorm column sums): only a fresh (zeroed, first-writer) slice."""
        return self.c[i][0] if self.c[i][1] == "fresh" else None

    def finish_overwrite(self, i, value):
        """value was computed by an overwriting kernel; returns what the backward node hands to autograd."""
        view, mode, ar, idx = self.c[i]
        if mode == "fresh":
            return ar.alias(idx)          # written in place
        if mode == "accum":
            view.add_(value)
            return None
        return value


def _wgrad(dy, x, weights, biases_present, need_w, need_b, launcher=None):
    """dW / db of the stacked segments into their arena slices (or fresh buffers); returns what autograd gets.
    launcher: linear_bwd_weight of dy's stream (default) or another launcher with its contract."""
    launcher = launcher or _ops(dy).linear_bwd_weight
    nseg, seg_n = len(weights), weights[0].shape[0]
    cw = _Claims(weights, need_w)
    cb = _Claims(biases_present, need_b)
    wanted = [c for c, n in zip(cw.c, need_w) if n] + [c for c, n in zip(cb.c, need_b) if n]
    side = _WGRAD["on"] and dy.is_cuda and len(wanted) > 0 and all(c[1] == "fresh" for c in wanted)
    if side:
        ws, cur = _wgrad_stream(dy.device, N.raw_stream(dy.device.index))
        ws.wait_stream(cur)
        N.set_stream(ws)
        try:
            dws, dbs = launcher(dy, x, nseg, seg_n, need_b, dw_out=cw.views(), db_out=cb.views())
        finally:
            N.set_stream(cur)
        dy.record_stream(ws)
        x.record_stream(ws)
        _WGRAD["used"].setdefault(dy.device.index, {})[ws.cuda_stream] = ws
        hold_for_side_stream(ws, dy)     # (dy may also be on its way back to autograd as the residual's gradient)
    else:
        dws, dbs = launcher(dy, x, nseg, seg_n, need_b, dw_out=cw.views(), db_out=cb.views())
    return ([cw.out(s, dws[s]) if need_w[s] else None for s in range(nseg)],
            [cb.out(s, dbs[s]) if need_b[s] else None for s in range(nseg)])


class LinearFn(Function):
    """y = dropout(act(x @ cat(W).T + cat(b)), p) (+ residual). Inputs: x, residual, act, nseg, drop_p, pad_cols, out_f32,
    W..., b... pad_cols (fp32 x): see ops.linear_fwd. out_f32 (bf16 x): y is fp32 (the image-feature projection in front of
    the fp32 embedding kernel, the poolers). A bf16 x comes without act, with GELU and a bf16 result, or with ReLU and an
    fp32 result (functional.linear runs every other such linear on the fp32 kernels).
    The dropout mask is regenerated in backward from the saved seed (vb_dropout on the incoming gradient)."""

    @staticmethod
    def forward(ctx, x, residual, act, nseg, drop_p, pad_cols, out_f32, *wb):
        weights, biases = list(wb[:nseg]), list(wb[nseg:])
        seed = next_seed() if drop_p > 0.0 else 0
        if x.dtype == BF16:
            # with an activation (functional.linear: GELU with a bf16 result, ReLU with an fp32 one - the prediction-head
            # transforms and the poolers): GELU saves gelu'(pre-activation) as FFNFn does, ReLU is masked by its output
            y, pre = ops16.linear_fwd(x, weights, biases, act, residual, drop_p=drop_p, seed=seed, out_f32=out_f32,
                                      want_act_grad=act == "gelu")
            if act == "relu":
                pre = y
        else:
            y, pre = ops.linear_fwd(x, weights, biases, act, residual, want_preact=act is not None, drop_p=drop_p,
                                    seed=seed, pad_cols=pad_cols)
        ctx.save_for_backward(x, pre, *weights, *[b for b in biases if b is not None])
        ctx.act, ctx.nseg = act, nseg
        ctx.drop = (drop_p, seed)
        ctx.has_bias = [b is not None for b in biases]
        return _tag_drop(y, drop_p, seed) if residual is not None and act is None else y

    @staticmethod
    def backward(ctx, dy):
        x, pre = ctx.saved_tensors[:2]
        nseg = ctx.nseg
        weights = list(ctx.saved_tensors[2:2 + nseg])
        rest = list(ctx.saved_tensors[2 + nseg:])
        biases = [rest.pop(0) if h else None for h in ctx.has_bias]
        seg_n, K = weights[0].shape[0], weights[0].shape[1]
        if dy.dtype != x.dtype:      # out_f32: the gradient of the fp32 output arrives in fp32
            if ctx.act == "relu":    # (the poolers) mask and rounding in one pass
                dy, pre = ops16.relu_bwd(dy, pre), None
            else:
                dy = ops16.cast_bf16(dy)
        elif x.dtype == BF16 or not (ops._row_strided(dy) and ctx.drop[0] == 0.0 and ctx.act is None
                                     and not ctx.needs_input_grad[1]):
            dy = dy.contiguous()     # (a row-strided gradient of padded fp32 logits feeds the GEMMs in place)
        dres = dy if ctx.needs_input_grad[1] else None
        if ctx.drop[0] > 0.0:
            dy = _dropped(dy, ctx.drop)
        if ctx.act is None or pre is None:
            dpre = dy
        elif x.dtype == BF16:        # GELU: pre is the saved derivative
            dpre = ops16.mul(dy.contiguous(), pre)
        else:
            dpre = ops.act_bwd(dy, pre, ctx.act)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _dgrad(dpre, weights, K).view(x.shape)
        need_w = [bool(ctx.needs_input_grad[7 + s]) for s in range(nseg)]
        need_b = [ctx.has_bias[s] and ctx.needs_input_grad[7 + nseg + s] for s in range(nseg)]
        dws, dbs = [None] * nseg, [None] * nseg
        if any(need_w) or any(need_b):
            # (the fused launch computes every segment; segments nobody asked for land in scratch buffers)
            launcher = None
            if (x.dtype != BF16 and nseg == 1 and dpre.is_cuda
                    and ops16.ragged_wgrad_ok(seg_n, K, dpre.numel() // max(seg_n, 1))):
                # bf16 mode: the wide ragged heads (30,522-wide MLM decoder) on the bf16 weight-gradient kernel
                launcher = lambda dy_, x_, nseg_, seg_n_, want_b, dw_out=None, db_out=None: \
                    ops16.linear_bwd_weight_ragged(dy_, x_, want_b, dw_out, db_out)
            dws, dbs = _wgrad(dpre, x, weights, biases, need_w, need_b, launcher)
        return (dx, dres, None, None, None, None, None) + tuple(dws) + tuple(dbs)


class RaggedLinearFn(Function):
    """y = x @ W.T + b for a bf16 x and a weight whose height n is no tile multiple (the tied 30,522-wide MLM decoder, the
    1,601-wide region decoder): the bf16 kernels on the zero-padded shadow (ops16.linear_ragged_*). y is an fp32 [rows, n] view
    of a [rows, n_pad] buffer. The output carries `_vb_ragged`: a loss node that reads it directly (CrossEntropyFn, KLDivFn)
    then hands over its gradient as the padded bf16 operands G (and G^T) these GEMMs take - a NaN placeholder travels through
    autograd in their place (`_vb_grad16`). Any other gradient arrives in fp32 and is rounded here. bias_grad_f32 (the decoders
    of VILBertForVLTasks, whose gradient always arrives that way): the bias gradient is then the fp32 column sum of that
    gradient BEFORE the rounding, left behind by the cast (ops16.cast_rows_colsum) - as the fp32-tensor path sums it; without
    it the weight-gradient kernel sums the rounded operand."""

    @staticmethod
    def forward(ctx, x, weight, bias, bias_grad_f32=False):
        y = ops16.linear_ragged_fwd(x, weight, bias)
        ctx.save_for_backward(x, weight, *([bias] if bias is not None else []))
        ctx.bias_grad_f32 = bool(bias_grad_f32)
        y._vb_ragged = True
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors[:2]
        bias = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        n, K = weight.shape
        rows = x.numel() // K
        n_pad = ops16.padded(n)
        tag = getattr(dy, "_vb_grad16", None)
        part = None
        if tag is not None and tag[0].shape == (rows, n_pad):
            G, GT, part = tag       # part: fp32 column sums of the unrounded loss gradient per 64 rows (cross entropy), or None
        else:
            dy2 = dy.reshape(rows, n)
            GT = None
            if ctx.bias_grad_f32 and bias is not None and ctx.needs_input_grad[2]:
                # with the fp32 column sums of the gradient from the same pass: the bias gradient is not summed from rounded values
                G, part = ops16.cast_rows_colsum(ops16.rows_addressable(dy2))
            else:
                G = ops16.cast_rows_padded(dy2)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops16.linear_ragged_bwd_input(G, GT, weight, bias, rows).view(x.shape)
        need_w = bool(ctx.needs_input_grad[1])
        need_b = bool(bias is not None and ctx.needs_input_grad[2])
        if need_b and part is not None:
            # the bias gradient in fp32 from the loss kernel's partial sums, not from the bf16-rounded G: the column sum of the
            # 30,522-wide decoder hardly depends on the logits, so the rounding of its ~rows terms would be its whole error
            cb = _Claims([bias], [True])
            db = cb.out(0, ops16.colsum_parts(part, n, cb.views()[0]))
            need_b = False
        if need_w or need_b:
            launcher = lambda dy_, x_, nseg_, seg_n_, want_b, dw_out=None, db_out=None: \
                ops16.linear_ragged_bwd_weight(dy_, x_, seg_n_, want_b, dw_out, db_out)
            (dw,), (db_w,) = _wgrad(G, x, [weight], [bias], [need_w], [need_b], launcher)
            db = db_w if need_b else db
        return dx, dw, db, None


class SkinnyLinearFn(Function):
    """y fp32 [..., n] = dropout(x, p) @ W.T + b + row_add for a bf16 x and n <= 4 outputs (`vision_logit`, `linguisic_logit` of
    VILBertForVLTasks; ops16.skinny_*): the dropped input is never materialised - forward, input gradient and weight gradient
    regenerate the mask from the saved (p, seed) over x itself. W is the fp32 master weight (no shadow). row_add (one fp32
    value per row, the additive region mask) gets no gradient. The weight gradient goes where LinearFn's goes (_wgrad: arena
    slices, side stream)."""

    @staticmethod
    def forward(ctx, x, weight, bias, row_add, drop_p):
        seed = next_seed() if drop_p > 0.0 else 0
        y = ops16.skinny_fwd(x, weight, bias, row_add, drop_p, seed)
        ctx.save_for_backward(x, weight, *([bias] if bias is not None else []))
        ctx.drop = (drop_p, seed)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors[:2]
        bias = ctx.saved_tensors[2] if len(ctx.saved_tensors) > 2 else None
        p, seed = ctx.drop
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = ops16.skinny_bwd_input(dy, weight, p, seed).view(x.shape)
        need_w = bool(ctx.needs_input_grad[1])
        need_b = bool(bias is not None and ctx.needs_input_grad[2])
        if need_w or need_b:
            launcher = lambda dy_, x_, nseg_, seg_n_, want_b, dw_out=None, db_out=None: \
                ops16.skinny_bwd_weight(dy_, x_, seg_n_, want_b[0], dw_out[0] if dw_out else None,
                                        db_out[0] if db_out else None, p, seed)
            (dw,), (db,) = _wgrad(dy, x, [weight], [bias], [need_w], [need_b], launcher)
        return dx, dw, db, None, None


def _grad16_placeholder(like, payload):
    """What a loss node returns to autograd in place of the fp32 gradient it did not compute: a [rows, n] fp32 view of ONE
    NaN (should anything but the ragged linear in front read it, the NaN shows) that carries the bf16 operands."""
    p = torch.full((1, 1), float("nan"), dtype=torch.float32, device=like.device).expand(like.shape)
    p._vb_grad16 = payload
    return p


class FFNFn(Function):
    """y = dropout(act(x @ W1.T + b1) @ W2.T + b2, p) + x - the feed-forward block in front of its LayerNorm
    (reference vilbert.py:500-503 + :513-517 and the image / connection twins), as ONE autograd node.
    Backward: the dgrad through W1 adds the skip-connection gradient in its GEMM epilogue (no torch add). The
    activation backward is fused too: the forward epilogue of the up-projection stores act'(pre-activation) next to
    the activation (one extra exp per element where erf is computed anyway) and the dgrad through W2 multiplies by
    it in its epilogue - no erf / exp in any backward kernel, no separate elementwise pass over [M, intermediate]."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, act, drop_p):
        seed = next_seed() if drop_p > 0.0 else 0
        h, dact = _ops(x).linear_fwd(x, [w1], [b1], act, None, want_act_grad=True)
        y, _ = _ops(x).linear_fwd(h, [w2], [b2], None, x, drop_p=drop_p, seed=seed)
        ctx.save_for_backward(x, dact, h, w1, w2, *[b for b in (b1, b2) if b is not None])
        ctx.act, ctx.drop = act, (drop_p, seed)
        ctx.has_bias = (b1 is not None, b2 is not None)
        return _tag_drop(y, drop_p, seed)

    @staticmethod
    def backward(ctx, dy):
        x, dact, h, w1, w2 = ctx.saved_tensors[:5]
        rest = list(ctx.saved_tensors[5:])
        b1 = rest.pop(0) if ctx.has_bias[0] else None
        b2 = rest.pop(0) if ctx.has_bias[1] else None
        dy = dy.contiguous()
        dyd = _dropped(dy, ctx.drop) if ctx.drop[0] > 0.0 else dy
        inter, hidden = w1.shape[0], w1.shape[1]
        dpre = _dgrad(dyd, [w2], inter, mul=dact)
        dw2 = db2 = dw1 = db1 = dx = None
        nb2 = bool(ctx.has_bias[1] and ctx.needs_input_grad[4])
        if ctx.needs_input_grad[3] or nb2:
            (dw2,), (db2,) = _wgrad(dyd, h, [w2], [b2], [bool(ctx.needs_input_grad[3])], [nb2])
        if ctx.needs_input_grad[0]:
            dx = _dgrad(dpre, [w1], hidden, residual=dy).view(x.shape)
        nb1 = bool(ctx.has_bias[0] and ctx.needs_input_grad[2])
        if ctx.needs_input_grad[1] or nb1:
            (dw1,), (db1,) = _wgrad(dpre, x, [w1], [b1], [bool(ctx.needs_input_grad[1])], [nb1])
        return dx, dw1, db1, dw2, db2, None, None


def _ln_bwd(dy, x, mean, rstd, gamma, beta, need_g, need_b, drop=None):
    """LayerNorm backward with dgamma / dbeta written straight into their arena slices when those are fresh.
    drop = (p, seed) of the dense layer in front: dx comes back tagged with its dropout-masked twin (see _DROP_HINT)."""
    c = _Claims([gamma, beta], [need_g, need_b])
    res = _ops(x).layernorm_bwd(dy, x, mean, rstd, gamma, c.fresh_or_none(0), c.fresh_or_none(1), drop=drop)
    dx, dgamma, dbeta = res[:3]
    if len(res) == 4:
        dx._vb_dropped = (drop[0], drop[1], res[3], dx.data_ptr(), dx._version)
    return dx, (c.finish_overwrite(0, dgamma) if need_g else None), (c.finish_overwrite(1, dbeta) if need_b else None)


# Dropout-mask hand-over between two autograd nodes (round 3, -66 launches per step). Every BertSelfOutput / BertOutput /
# BertBiOutput is y = LayerNorm(dropout(dense(h), p) + x): LinearFn / FFNFn produce the pre-LayerNorm sum, LayerNormFn
# consumes it. In backward the LayerNorm node computes dx and the dense node needs dropout(dx) - the same elements, the
# mask is a function of (seed, index). The forward of the dense node tags its output tensor with (p, seed)
# (`_vb_drop`), LayerNormFn.forward copies the tag into its context, its backward lets the LayerNorm kernel write the
# masked gradient next to dx and tags dx with it (`_vb_dropped`), the dense node's backward uses the twin when the tag
# matches its own (p, seed). Pure optimisation: without a matching tag every node falls back to its own vb_dropout.
def _tag_drop(y, drop_p, seed):
    if drop_p > 0.0:
        y._vb_drop = (drop_p, seed)
    return y


def _dropped(dy, drop):
    """dropout(dy) for the dense node's backward: the twin the LayerNorm kernel already wrote, or a vb_dropout launch."""
    tag = getattr(dy, "_vb_dropped", None)
    # the twin equals dropout(dy) only while dy still IS the tensor the LayerNorm kernel wrote: same storage and no
    # in-place write since (autograd's InputBuffer may accumulate a second consumer's gradient in place into a tensor it
    # holds the only reference to - the Python attribute would survive that, the version counter does not)
    if (tag is not None and tag[0] == drop[0] and tag[1] == drop[1] and tag[2].shape == dy.shape
            and tag[3] == dy.data_ptr() and tag[4] == dy._version):
        return tag[2]
    return _ops(dy).dropout(dy, drop[0], drop[1])


class LayerNormFn(Function):
    """TF-style LayerNorm of one tensor (statistics fp32 on both streams)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        y, mean, rstd = _ops(x).layernorm_fwd(x, gamma, beta, eps, want_stats=True)
        ctx.save_for_backward(x, mean, rstd, gamma, beta)
        ctx.drop_hint = getattr(x, "_vb_drop", None)      # x = dropout(dense(h)) + residual of the node in front
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, rstd, gamma, beta = ctx.saved_tensors
        dx, dgamma, dbeta = _ln_bwd(dy, x, mean, rstd, gamma, beta, ctx.needs_input_grad[1], ctx.needs_input_grad[2],
                                    drop=ctx.drop_hint)
        out = dx.view(x.shape)
        tag = getattr(dx, "_vb_dropped", None)
        if tag is not None:
            out._vb_dropped = (tag[0], tag[1], tag[2].view(x.shape), out.data_ptr(), out._version)
        return out, dgamma, dbeta, None


class DropoutFn(Function):
    """y = dropout(x, p) (+ residual)."""

    @staticmethod
    def forward(ctx, x, residual, p):
        ctx.p, ctx.seed = p, next_seed()
        return ops.dropout(x, p, ctx.seed, residual)

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = ops.dropout(dy, ctx.p, ctx.seed) if ctx.needs_input_grad[0] else None
        return dx, (dy if ctx.needs_input_grad[1] else None), None


def dropout(x, p, residual=None):
    return DropoutFn.apply(x, residual, p)


def _check_keys_for_backward(n_keys, want_probs):
    """More than ops.MAX_KEYS keys run chunk by chunk, forward and backward (ops._attention_fwd_long / _attention_bwd_long);
    only the probabilities tensor (`visualization`) does not exist there - say so where the call is made."""
    if n_keys > ops.MAX_KEYS and want_probs:
        raise RuntimeError("attention: %d keys with attention maps - one launch serves at most %d keys, and the chunked path "
                           "of longer key sequences (stacked retrieval options, in_batch_pairs) returns no probabilities"
                           % (n_keys, ops.MAX_KEYS))


class SelfAttnFn(Function):
    """ctx = attention over one fused [q | k | v] projection; dqkv is written in one buffer."""

    @staticmethod
    def forward(ctx, qkv, mask_add, heads, drop_p, want_probs):
        H = qkv.shape[-1] // 3
        _check_keys_for_backward(qkv.shape[1], want_probs)
        seed = next_seed() if drop_p > 0.0 else 0
        out, probs, lse = attention_fwd(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], mask_add, heads, want_probs,
                                        True, drop_p, seed)
        ctx.save_for_backward(qkv, mask_add, lse)
        ctx.meta = (heads, drop_p, seed)
        if probs is None:                     # (none on the bf16 stream)
            probs = qkv.new_empty(0)
        ctx.mark_non_differentiable(probs)
        ctx.set_materialize_grads(False)      # no zeros() for the gradient slot of the non-differentiable probs
        return out, probs

    @staticmethod
    def backward(ctx, d_out, _d_probs):
        qkv, mask_add, lse = ctx.saved_tensors
        if d_out is None:
            return None, None, None, None, None
        heads, drop_p, seed = ctx.meta
        H = qkv.shape[-1] // 3
        dqkv = torch.empty_like(qkv)
        _ops(qkv).attention_bwd(d_out, qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], mask_add, heads, lse,
                                dqkv[..., :H], dqkv[..., H:2 * H], dqkv[..., 2 * H:], drop_p, seed)
        return dqkv, None, None, None, None


class BiAttnFn(Function):
    """Both directions of the co-attention (reference vilbert.py:768-809) over the two fused projections:
    ctx1 = attn(q2; k1, v1 | mask1) for the text stream, ctx2 = attn(q1; k2, v2 | mask2) for the image
    stream. The backward fills dqkv1 / dqkv2 with each slice written exactly once."""

    @staticmethod
    def forward(ctx, qkv1, qkv2, mask1, mask2, heads, p1, p2, want_probs):
        H = qkv1.shape[-1] // 3
        _check_keys_for_backward(max(qkv1.shape[1], qkv2.shape[1]), want_probs)
        s1 = next_seed() if p1 > 0.0 else 0
        s2 = next_seed() if p2 > 0.0 else 0
        q1, k1, v1 = qkv1[..., :H], qkv1[..., H:2 * H], qkv1[..., 2 * H:]
        q2, k2, v2 = qkv2[..., :H], qkv2[..., H:2 * H], qkv2[..., 2 * H:]
        ctx1, probs1, lse1 = attention_fwd(q2, k1, v1, mask1, heads, want_probs, True, p1, s1)
        ctx2, probs2, lse2 = attention_fwd(q1, k2, v2, mask2, heads, want_probs, True, p2, s2)
        ctx.save_for_backward(qkv1, qkv2, mask1, mask2, lse1, lse2)
        ctx.meta = (heads, p1, p2, s1, s2)
        ctx.out_shapes = (ctx1.shape, ctx2.shape)      # (a batch of 1 broadcasts against the other stream's)
        if probs1 is None:
            probs1, probs2 = qkv1.new_empty(0), qkv1.new_empty(0)
        ctx.mark_non_differentiable(probs1, probs2)
        ctx.set_materialize_grads(False)
        return ctx1, ctx2, probs1, probs2

    @staticmethod
    def backward(ctx, d1, d2, _dp1, _dp2):
        qkv1, qkv2, mask1, mask2, lse1, lse2 = ctx.saved_tensors
        heads, p1, p2, s1, s2 = ctx.meta
        if d1 is None and d2 is None:
            return (None,) * 8
        if d1 is None:                         # only one direction reached the loss: the other one's gradient is zero
            d1 = qkv1.new_zeros(ctx.out_shapes[0])
        if d2 is None:
            d2 = qkv1.new_zeros(ctx.out_shapes[1])
        H = qkv1.shape[-1] // 3
        sl = lambda t: (t[..., :H], t[..., H:2 * H], t[..., 2 * H:])
        q1, k1, v1 = sl(qkv1)
        q2, k2, v2 = sl(qkv2)
        dqkv1, dqkv2 = torch.empty_like(qkv1), torch.empty_like(qkv2)
        dq1, dk1, dv1 = sl(dqkv1)
        dq2, dk2, dv2 = sl(dqkv2)
        _ops(qkv1).attention_bwd(d1, q2, k1, v1, mask1, heads, lse1, dq2, dk1, dv1, p1, s1)
        _ops(qkv1).attention_bwd(d2, q1, k2, v2, mask2, heads, lse2, dq1, dk2, dv2, p2, s2)
        return dqkv1, dqkv2, None, None, None, None, None, None


class TextEmbedFn(Function):
    @staticmethod
    def forward(ctx, ids, seg, word, pos, typ, gamma, beta, eps, task_ids, task_emb):
        out, mean, rstd, presum = ops.text_embed_ln_fwd(ids, seg, word, pos, typ, gamma, beta, eps, task_ids,
                                                        task_emb, want_stats=True)
        ctx.save_for_backward(ids, seg, task_ids, presum, mean, rstd, gamma, beta, word, pos, typ, task_emb)
        return out

    @staticmethod
    def backward(ctx, dy):
        ids, seg, task_ids, presum, mean, rstd, gamma, beta, word, pos, typ, task_emb = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx, dgamma, dbeta = _ln_bwd(dy, presum, mean, rstd, gamma, beta, need[5], need[6])
        tables = [word, pos, typ, task_emb]
        want = [bool(need[2]), bool(need[3]), bool(need[4]), bool(task_emb is not None and need[9])]
        c = _Claims(tables, want)
        got = ops.text_embed_bwd(dx, ids, seg, task_ids, tuple(word.shape), tuple(pos.shape), tuple(typ.shape),
                                 tuple(task_emb.shape) if task_emb is not None else None, out=c.views())
        dword, dpos, dtype, dtask = [(c.out(i, got[i]) if want[i] else None) for i in range(4)]
        return None, None, dword, dpos, dtype, dgamma, dbeta, None, None, dtask


class ImageEmbedFn(Function):
    @staticmethod
    def forward(ctx, feat_proj, loc, w_loc, b_loc, gamma, beta, eps):
        out, mean, rstd, presum = ops.image_embed_ln_fwd(feat_proj, loc, w_loc, b_loc, gamma, beta, eps,
                                                         want_stats=True)
        ctx.save_for_backward(loc, presum, mean, rstd, gamma, beta, w_loc, b_loc)
        return out

    @staticmethod
    def backward(ctx, dy):
        loc, presum, mean, rstd, gamma, beta, w_loc, b_loc = ctx.saved_tensors
        need = ctx.needs_input_grad
        dsum, dgamma, dbeta = _ln_bwd(dy, presum, mean, rstd, gamma, beta, need[4], need[5])
        (dw_loc,), (db_loc,) = _wgrad(dsum, loc.reshape(-1, 5), [w_loc], [b_loc], [bool(need[2])], [bool(need[3])])
        return dsum, None, dw_loc, db_loc, dgamma, dbeta, None


class JointEmbedFn(Function):
    """The single-stream baseline's embedding (ops.joint_embed): one [B, T + R, H] buffer for both segments and the additive
    mask of the two masks. Inputs: ids, seg, word, pos, typ, gamma_t, beta_t, feat_proj, loc, w_loc, b_loc, typ_v (the image
    token-type TABLE; row 1 is added to every region, basebert.py:726-728), gamma_v, beta_v, eps, mask_t, mask_v. The three
    text tables and the image token-type table are padding_idx = 0 tables (reference basebert.py:290-298, :332-334): their
    rows 0 get no gradient from the gather - word row 0 still gets the tied decoder's."""

    @staticmethod
    def forward(ctx, ids, seg, word, pos, typ, gamma_t, beta_t, feat_proj, loc, w_loc, b_loc, typ_v, gamma_v, beta_v, eps,
                mask_t, mask_v):
        out, add_mask, mean, rstd, presum = ops.joint_embed(ids, seg, word, pos, typ, gamma_t, beta_t, feat_proj, loc, w_loc,
                                                            b_loc, typ_v[1], gamma_v, beta_v, eps, mask_t, mask_v,
                                                            want_stats=True)
        ctx.save_for_backward(ids, seg, loc, presum, mean, rstd, word, pos, typ, gamma_t, beta_t, w_loc, b_loc, typ_v,
                              gamma_v, beta_v)
        ctx.mark_non_differentiable(add_mask)
        ctx.set_materialize_grads(False)
        return out, add_mask

    @staticmethod
    def backward(ctx, dy, _d_mask):
        (ids, seg, loc, presum, mean, rstd, word, pos, typ, gamma_t, beta_t, w_loc, b_loc, typ_v, gamma_v,
         beta_v) = ctx.saved_tensors
        if dy is None:
            return (None,) * 17
        need = ctx.needs_input_grad
        ln = _Claims([gamma_t, beta_t, gamma_v, beta_v], [need[5], need[6], need[12], need[13]])
        dx_t, dx_v, dg_t, db_t, dg_v, db_v = ops.joint_embed_bwd(dy, presum, mean, rstd, gamma_t, gamma_v, ids.shape[1],
                                                                 *[ln.fresh_or_none(i) for i in range(4)])
        sums = [(ln.finish_overwrite(i, v) if w else None)
                for i, (v, w) in enumerate(zip((dg_t, db_t, dg_v, db_v), (need[5], need[6], need[12], need[13])))]
        want = [bool(need[2]), bool(need[3]), bool(need[4]), False]
        c = _Claims([word, pos, typ, None], want)
        got = ops.text_embed_bwd(dx_t, ids, seg, None, tuple(word.shape), tuple(pos.shape), tuple(typ.shape), None,
                                 out=c.views(), skip_rows0=(True, True))
        dword, dpos, dtype = [(c.out(i, got[i]) if want[i] else None) for i in range(3)]
        # the region rows: dx_v IS the gradient of the projected features (the feature projection's own node turns it into its
        # weight / bias gradients); the 5-wide location projection goes through the skinny weight-gradient path, and its bias
        # gradient colsum(dx_v) is also the gradient of row 1 of the image token-type table (row 0, the padding row, gets none)
        want_row = bool(need[11])
        (dw_loc,), (db_loc,) = ops.linear_bwd_weight(dx_v, loc.reshape(-1, 5), 1, w_loc.shape[0], [True])
        cv = _Claims([w_loc, b_loc, typ_v], [bool(need[9]), bool(need[10]), want_row])

        def into(i, value, row=None):
            """`value` added into parameter i's arena slice (zero-filled, or holding an earlier contribution) - into row `row` of it
            for the token-type table; without a slice the value itself (the table: zeros around its row)."""
            view = cv.c[i][0]
            if view is not None:
                (view if row is None else view[row]).add_(value)
                return cv.out(i, None)
            if row is None:
                return value
            table = torch.zeros_like(typ_v)
            table[row].copy_(value)
            return table

        B, S, H = presum.shape
        return (None, None, dword, dpos, dtype, sums[0], sums[1], dx_v.view(B, S - ids.shape[1], H), None,
                into(0, dw_loc) if need[9] else None, into(1, db_loc) if need[10] else None,
                into(2, db_loc, row=1) if want_row else None, sums[2], sums[3], None, None, None)


class TanhFn(Function):
    """y = tanh(x) on the pooler's [B, H] output (vbb_tanh_fwd / vbb_tanh_bwd)."""

    @staticmethod
    def forward(ctx, x):
        y = ops.tanh(x)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return ops.tanh_bwd(dy, y)


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss(ignore_index) (mean over counted rows) - reference vilbert.py:1453,1578-1585."""

    @staticmethod
    def forward(ctx, logits, labels, ignore_index):
        loss, lse, count = ops.xent_fwd(logits, labels, ignore_index)
        ctx.save_for_backward(logits, labels, lse, count)
        ctx.ignore_index = ignore_index
        ctx.to16 = bool(getattr(logits, "_vb_ragged", False))      # the logits of a RaggedLinearFn, read here directly
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        logits, labels, lse, count = ctx.saved_tensors
        if ctx.to16:
            want_t = ops16.padded(logits.shape[1]) >= ops16.WGRAD_FORM_MIN_WIDTH
            return _grad16_placeholder(logits, ops16.xent_bwd16(grad_loss, logits, labels, ctx.ignore_index, lse, count,
                                                                want_t, want_colsum=True)), None, None
        return ops.xent_bwd(grad_loss, logits, labels, ctx.ignore_index, lse, count), None, None


class KLDivFn(torch.autograd.Function):
    """sum(KLDivLoss(reduction="none")(log_softmax(scores), target)) / divisor - reference :1454,1516-1522."""

    @staticmethod
    def forward(ctx, scores, target, divisor):
        loss, lse, tsum = ops.kl_fwd(scores, target, divisor)
        ctx.save_for_backward(scores, target, lse, tsum)
        ctx.divisor = divisor
        ctx.to16 = bool(getattr(scores, "_vb_ragged", False))
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        scores, target, lse, tsum = ctx.saved_tensors
        if ctx.to16:
            return _grad16_placeholder(scores, (ops16.kl_bwd16(grad_loss, scores, target, lse, tsum, ctx.divisor), None, None)), \
                None, None
        return ops.kl_bwd(grad_loss, scores, target, lse, tsum, ctx.divisor), None, None


class BCEWithLogitsFn(torch.autograd.Function):
    """nn.BCEWithLogitsLoss(reduction="mean") - reference task_utils.py:25-28, 325-374. Nothing but the two operands is
    saved (the backward recomputes the sigmoid); the target gets no gradient."""

    @staticmethod
    def forward(ctx, logits, target):
        ctx.save_for_backward(logits, target)
        return ops.bce_fwd(logits, target)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        logits, target = ctx.saved_tensors
        return ops.bce_bwd(grad_loss, logits, target), None


class NCERegionFn(torch.autograd.Function):
    """NCE masked-region loss, visual_target == 2 - reference :1523-1575. The negatives are a pure function of (seed, labelled
    region, draw) (csrc/nce_index.h); the seed is drawn from next_seed() unless given and kept on the node. The forward
    leaves the unscaled gradient behind (ops.nce_fwd), so the backward is one scale; the target table gets no gradient."""

    @staticmethod
    def forward(ctx, predict, table, idx_r, valid, count, batch, regions, n_across, n_inside, seed=None):
        seed = next_seed() if seed is None else seed
        neg = ops.nce_negatives(idx_r, batch, regions, n_across, n_inside, seed)
        loss, dsave = ops.nce_fwd(predict, table, idx_r, neg, valid, count, want_grad=True)
        ctx.seed = seed
        ctx.valid = valid
        ctx.save_for_backward(dsave, count)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        dsave, count = ctx.saved_tensors
        return (ops.nce_bwd(grad_loss, dsave, ctx.valid, count),) + (None,) * 9


class GatherRows16Fn(Function):
    """compact[r] = src[row_map[r]] on bf16 rows (vilbert.py `_head_row_maps` / `_row_map`: the rows of an encoder output the poolers and a
    prediction head read; -1 = a zero padding row). Backward: ONE scatter of the compact gradient into the bf16 gradient of
    the whole [rows, H] tensor - every row written once, zeros where no compact row stands for it."""

    @staticmethod
    def forward(ctx, src, row_map):
        ctx.save_for_backward(row_map)
        ctx.full_rows = src.shape[0]
        return ops16.gather_rows(src, row_map)

    @staticmethod
    def backward(ctx, d):
        (row_map,) = ctx.saved_tensors
        return ops16.scatter_rows(d.contiguous(), row_map, ctx.full_rows), None


class CastFn(Function):
    """fp32 <-> bfloat16 at the edges of the bf16 stream (embeddings in, sequence outputs out); backward = the other cast."""

    @staticmethod
    def forward(ctx, x, to_bf16):
        ctx.to_bf16 = to_bf16
        return ops16.cast_bf16(x) if to_bf16 else ops16.cast_f32(x)

    @staticmethod
    def backward(ctx, dy):
        return (ops16.cast_f32(dy) if ctx.to_bf16 else ops16.cast_bf16(dy)), None
