"""Fused ops of the model, autograd-visible.

When no input needs a gradient (or grad mode is off) the forward launcher is called directly with
nothing saved; otherwise the op goes through its ``torch.autograd.Function`` (autograd_ops.py), whose
backward also runs native kernels only.
"""
import torch

from . import _native as N
from . import autograd_ops as A
from . import ops
from . import ops16

BF16 = torch.bfloat16


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


# ---------------------------------------------------------------------------------------------------------------
# bf16 stream (round 5, _native.bf16_stream()): between the embeddings and the poolers / heads the hidden states are
# bfloat16 tensors; every op below dispatches on the dtype of its input. A shape the bf16 kernels do not serve (the tiny
# test configurations, an activation other than GELU inside an FFN, attention probabilities wanted) goes through the fp32
# kernels between two casts - same stream dtype on both sides, so the layers around it never notice.
# ---------------------------------------------------------------------------------------------------------------
def _is16(x):
    return torch.is_tensor(x) and x.dtype == BF16 and N.bf16_stream()


def to_bf16(x):
    if x.dtype == BF16:
        return x
    return A.CastFn.apply(x, True) if _needs_grad(x) else ops16.cast_bf16(x)


def to_f32(x):
    if x is None or x.dtype != BF16:
        return x
    return A.CastFn.apply(x, False) if _needs_grad(x) else ops16.cast_f32(x)


def gather_rows16(src, row_map):
    """bf16 [M, H] = src[row_map] (src bf16 [rows, H], row_map int32 [M], -1 = zero row); backward scatters once."""
    return A.GatherRows16Fn.apply(src, row_map) if _needs_grad(src) else ops16.gather_rows(src, row_map)


def _uniform_bias(biases):
    return all(b is None for b in biases) or all(b is not None for b in biases)


def linear(x, weights, biases=None, act=None, residual=None, drop_p=0.0, pad_cols=False, out="f32", out_f32=False,
           bias_grad_f32=False):
    """dropout(act(x @ cat(weights).T + cat(biases)), drop_p) (+ residual); weights / biases may be single
    tensors; drop_p is the EFFECTIVE probability (0 in eval mode). pad_cols, out: see ops.linear_fwd (out is a request
    the MX inference mode honours where the shape allows it; everywhere else the result is an fp32 tensor). On the bf16
    stream the result is bf16, or fp32 with out_f32. bias_grad_f32: autograd_ops.RaggedLinearFn (a decoder of ragged width
    on the bf16 stream). It is IGNORED everywhere else - in particular for a decoder whose width is a tile multiple, which takes
    the LinearFn route and sums its bias gradient from the bf16-rounded gradient."""
    if not isinstance(weights, (list, tuple)):
        weights, biases = [weights], [biases]
    if biases is None:
        biases = [None] * len(weights)
    grad = _needs_grad(x, residual, *weights, *biases)
    kern = ops
    if _is16(x):
        seg_n, K = weights[0].shape
        base = x.is_cuda and _uniform_bias(biases) and (residual is None or residual.dtype == BF16)
        ok = base and ops16.eligible(K, len(weights) * seg_n, seg_n, act)
        if (not ok and base and out_f32 and len(weights) == 1 and act is None and residual is None and drop_p == 0.0
                and ops16.ragged_ok(K, seg_n)):
            # an output width that is no tile multiple (the 30,522-wide MLM decoder, the 1,601-wide region decoder): the bf16
            # kernels on a zero-padded shadow, fp32 result
            if grad:
                return A.RaggedLinearFn.apply(x, weights[0], biases[0], bias_grad_f32)
            return ops16.linear_ragged_fwd(x, weights[0], biases[0])
        # under autograd an activation stays on the bf16 kernels where its backward has one: GELU with a bf16 result (the
        # saved derivative is multiplied in), ReLU with an fp32 result (masked by the output); swish, and VB_BF16_HEADS=0,
        # take the fp32 kernels
        act16 = (ops16.heads_enabled() and residual is None and drop_p == 0.0
                 and ((act == "gelu" and not out_f32) or (act == "relu" and out_f32)))
        if not ok or (grad and act is not None and not act16):
            y = linear(to_f32(x), weights, biases, act, to_f32(residual), drop_p)
            return y if out_f32 else to_bf16(y)
        kern = ops16
    if grad:
        return A.LinearFn.apply(x, residual, act, len(weights), drop_p, pad_cols, out_f32, *weights, *biases)
    seed = A.next_seed() if drop_p > 0.0 else 0
    if kern is ops16:
        return ops16.linear_fwd(x, weights, biases, act, residual, drop_p=drop_p, seed=seed, out_f32=out_f32)[0]
    return ops.linear_fwd(x, weights, biases, act, residual, drop_p=drop_p, seed=seed, pad_cols=pad_cols, out=out)[0]


def skinny_linear(x, weight, bias=None, row_add=None, drop_p=0.0):
    """dropout(x, drop_p) @ weight.T + bias + row_add[..., None] -> fp32 [..., n] for a bf16 x and a weight of 1 .. 4 rows
    (ops16.skinny_ok): the dropout is drawn inside the kernels, drop_p is the EFFECTIVE probability."""
    if _needs_grad(x, weight, bias):
        return A.SkinnyLinearFn.apply(x, weight, bias, row_add, drop_p)
    return ops16.skinny_fwd(x, weight, bias, row_add, drop_p, A.next_seed() if drop_p > 0.0 else 0)


def linear_f32_out(x, weight, bias):
    """x bf16 -> fp32 result (the 2048 -> 1024 region-feature projection in front of the fp32 embedding kernel)."""
    return linear(x, weight, bias, out_f32=True)


def ffn(x, w1, b1, act, w2, b2, drop_p=0.0):
    """dropout(act(x @ w1.T + b1) @ w2.T + b2, drop_p) + x  (the block in front of the output LayerNorm)."""
    kern = ops
    if _is16(x):
        ok = (act == "gelu" and x.is_cuda and ops16.eligible(w1.shape[1], w1.shape[0]) and ops16.eligible(w2.shape[1], w2.shape[0])
              and _uniform_bias([b1]) and _uniform_bias([b2]))
        if not ok:
            return to_bf16(ffn(to_f32(x), w1, b1, act, w2, b2, drop_p))
        kern = ops16
    if _needs_grad(x, w1, b1, w2, b2):
        return A.FFNFn.apply(x, w1, b1, w2, b2, act, drop_p)
    if kern is ops16:
        h = ops16.linear_fwd(x, [w1], [b1], act)[0]
        seed = A.next_seed() if drop_p > 0.0 else 0
        return ops16.linear_fwd(h, [w2], [b2], None, x, drop_p=drop_p, seed=seed)[0]
    # MX mode (inference): the activation of the up-projection leaves its GEMM as MX codes for the down-projection - it is
    # never written in fp32 and never re-read by a quantiser
    mx = (drop_p == 0.0 and ops.mx_eligible(w1.shape[1], w1.shape[0], act, biases=[b1])
          and ops.mx_eligible(w2.shape[1], w2.shape[0], None, biases=[b2]) and x.is_cuda)
    h = ops.linear_fwd(x, [w1], [b1], act, out="mx" if mx else "f32")[0]
    seed = A.next_seed() if drop_p > 0.0 else 0
    return ops.linear_fwd(h, [w2], [b2], None, x, drop_p=drop_p, seed=seed, out="bf16" if mx and ops.mx_stream_bf16() else "f32")[0]


def layer_norm(x, gamma, beta, eps=1e-12):
    kern = ops
    if _is16(x):
        if x.shape[-1] > 1024 or x.shape[-1] % 4 != 0 or not x.is_cuda:
            return to_bf16(layer_norm(to_f32(x), gamma, beta, eps))
        kern = ops16
    if _needs_grad(x, gamma, beta):
        return A.LayerNormFn.apply(x, gamma, beta, eps)
    return kern.layernorm_fwd(x, gamma, beta, eps)[0]


def dropout(x, p, residual=None):
    """dropout(x, p) (+ residual); p is the EFFECTIVE probability (0 in eval mode)."""
    if p <= 0.0:
        # identity (+ residual): the callers fuse the residual into the producing GEMM instead
        assert residual is None
        return x
    if _needs_grad(x, residual):
        return A.dropout(x, p, residual)
    return ops.dropout(x, p, A.next_seed(), residual)


def self_attention(qkv, mask_add, heads, drop_p=0.0, want_probs=False):
    """Attention over a fused [B, S, 3H] = [q | k | v] projection. Returns (context [B,S,H], probs|None)."""
    H = qkv.shape[-1] // 3
    bf16 = _is16(qkv)
    if bf16 and (want_probs or qkv.shape[1] > ops.MAX_KEYS or (H // heads) not in (32, 64, 128) or not qkv.is_cuda):
        ctx, probs = self_attention(to_f32(qkv), mask_add, heads, drop_p, want_probs)
        return to_bf16(ctx), probs
    if _needs_grad(qkv):
        out, probs = A.SelfAttnFn.apply(qkv, mask_add, heads, drop_p, want_probs)
        return out, (probs if want_probs else None)
    if not bf16 and qkv.dtype == BF16:     # MX inference mode: bf16 projection in, MX context out (ops.mx_attention_ok held)
        return ops.attention_fwd_mx_any(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], mask_add, heads), None
    seed = A.next_seed() if drop_p > 0.0 else 0
    out, probs, _ = A.attention_fwd(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], mask_add, heads,
                                    want_probs, False, drop_p, seed)
    return out, probs


def bi_attention(qkv1, qkv2, mask1, mask2, heads, p1=0.0, p2=0.0, want_probs=False):
    """Co-attention between stream 1 (image, qkv1 / mask1) and stream 2 (text, qkv2 / mask2):
    returns (ctx1 = attn(q2; k1, v1), ctx2 = attn(q1; k2, v2), probs1|None, probs2|None)."""
    H = qkv1.shape[-1] // 3
    bf16 = _is16(qkv1) or _is16(qkv2)
    if bf16 and (want_probs or max(qkv1.shape[1], qkv2.shape[1]) > ops.MAX_KEYS or (H // heads) not in (32, 64, 128)
                 or not (qkv1.is_cuda and _is16(qkv1) and _is16(qkv2))):
        c1, c2, pr1, pr2 = bi_attention(to_f32(qkv1), to_f32(qkv2), mask1, mask2, heads, p1, p2, want_probs)
        return to_bf16(c1), to_bf16(c2), pr1, pr2
    if _needs_grad(qkv1, qkv2):
        c1, c2, pr1, pr2 = A.BiAttnFn.apply(qkv1, qkv2, mask1, mask2, heads, p1, p2, want_probs)
        return c1, c2, (pr1 if want_probs else None), (pr2 if want_probs else None)
    if not bf16 and qkv1.dtype == BF16 and qkv2.dtype == BF16:
        c1 = ops.attention_fwd_mx_any(qkv2[..., :H], qkv1[..., H:2 * H], qkv1[..., 2 * H:], mask1, heads)
        c2 = ops.attention_fwd_mx_any(qkv1[..., :H], qkv2[..., H:2 * H], qkv2[..., 2 * H:], mask2, heads)
        return c1, c2, None, None
    s1 = A.next_seed() if p1 > 0.0 else 0
    s2 = A.next_seed() if p2 > 0.0 else 0
    c1, pr1, _ = A.attention_fwd(qkv2[..., :H], qkv1[..., H:2 * H], qkv1[..., 2 * H:], mask1, heads,
                                 want_probs, False, p1, s1)
    c2, pr2, _ = A.attention_fwd(qkv1[..., :H], qkv2[..., H:2 * H], qkv2[..., 2 * H:], mask2, heads,
                                 want_probs, False, p2, s2)
    return c1, c2, pr1, pr2


def text_embed_ln(ids, seg, word, pos, typ, gamma, beta, eps, task_ids=None, task_emb=None):
    if _needs_grad(word, pos, typ, gamma, beta, task_emb):
        return A.TextEmbedFn.apply(ids, seg, word, pos, typ, gamma, beta, eps, task_ids, task_emb)
    return ops.text_embed_ln_fwd(ids, seg, word, pos, typ, gamma, beta, eps, task_ids, task_emb)[0]


def image_embed_ln(feat_proj, loc, w_loc, b_loc, gamma, beta, eps):
    if _needs_grad(feat_proj, w_loc, b_loc, gamma, beta):
        return A.ImageEmbedFn.apply(feat_proj, loc, w_loc, b_loc, gamma, beta, eps)
    return ops.image_embed_ln_fwd(feat_proj, loc, w_loc, b_loc, gamma, beta, eps)[0]


def joint_embed_ln(ids, seg, word, pos, typ, gamma_t, beta_t, feat_proj, loc, w_loc, b_loc, typ_v, gamma_v, beta_v, eps,
                   mask_t=None, mask_v=None):
    """The single-stream baseline's embedding -> (states [B, T + R, H], additive mask [B, T + R]): text rows word + position +
    type under the text LayerNorm, image rows feat_proj + typ_v[1] + location projection under the image LayerNorm, and
    (1 - mask) * -10000 of the two masks (None = all ones), in one launch."""
    if _needs_grad(word, pos, typ, gamma_t, beta_t, feat_proj, w_loc, b_loc, typ_v, gamma_v, beta_v):
        return A.JointEmbedFn.apply(ids, seg, word, pos, typ, gamma_t, beta_t, feat_proj, loc, w_loc, b_loc, typ_v, gamma_v,
                                    beta_v, eps, mask_t, mask_v)
    return ops.joint_embed(ids, seg, word, pos, typ, gamma_t, beta_t, feat_proj, loc, w_loc, b_loc, typ_v[1], gamma_v, beta_v,
                           eps, mask_t, mask_v)[:2]


def tanh(x):
    return A.TanhFn.apply(x) if _needs_grad(x) else ops.tanh(x)


def cross_entropy(logits, labels, ignore_index=-1):
    """nn.CrossEntropyLoss(ignore_index=...)(logits [rows, n], labels [rows]) -> 0-dim loss."""
    if _needs_grad(logits):
        return A.CrossEntropyFn.apply(logits, labels, ignore_index)
    return ops.xent_fwd(logits, labels, ignore_index)[0]


def kl_div_log_softmax(scores, target, divisor):
    """sum(nn.KLDivLoss(reduction="none")(log_softmax(scores, 1), target)) / divisor -> 0-dim loss."""
    if _needs_grad(scores):
        return A.KLDivFn.apply(scores, target, divisor)
    return ops.kl_fwd(scores, target, divisor)[0]


def nce_region_loss(predict_rows, image_target, idx_r, valid_r, count, batch, regions, n_across, n_inside, seed=None):
    """NCE masked-region loss (visual_target == 2, reference vilbert.py:1523-1575) -> 0-dim loss. predict_rows [rows, dim]: the
    image head's output at the labelled regions idx_r (= b * regions + r, regions without the global row); image_target: the
    [batch, regions, dim] (or flat [batch * regions, dim]) target features, no gradient; valid_r: bool flag per row or None
    (padding rows of the fixed-capacity gather); count: 1-element fp32 device tensor, the divisor. Each row is contrasted with
    n_across regions of other samples and n_inside other regions of its own sample, drawn by csrc/nce_index.h from `seed`
    (default: autograd_ops.next_seed()) and the registered device step counter."""
    table = image_target.reshape(-1, image_target.size(-1))
    if table.size(0) != batch * regions:
        raise RuntimeError("nce_region_loss: image_target does not hold batch * regions rows")
    if _needs_grad(predict_rows):
        return A.NCERegionFn.apply(predict_rows, table, idx_r, valid_r, count, batch, regions, n_across, n_inside, seed)
    seed = A.next_seed() if seed is None else seed
    neg = ops.nce_negatives(idx_r, batch, regions, n_across, n_inside, seed)
    return ops.nce_fwd(predict_rows, table, idx_r, neg, valid_r, count, want_grad=False)[0]
