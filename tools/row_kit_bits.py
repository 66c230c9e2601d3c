"""SHA-256 of every output buffer of the head / loss row kernels (csrc/row_kit.h and the kernels built on it: bf16_helpers.hip,
heads16.hip, finetune16.hip, rowmap.hip, loss.hip, task_loss.hip, nce.hip) over fixed seeds - run it on two builds of the
library (--lib other.so) and diff the outputs: identical lines = identical bits. Every shape is the smallest that crosses a
boundary of its kernel (a 64-row tile, a 64-column tile, the 8-column chunk and its guarded tail, the 256-column row rule of
the task losses, a second block). Inputs come from seeds; nothing outside the tree is read."""
import argparse
import hashlib
import itertools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "vilbert-multi-task_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None, help="another build of libvilbert_hip.so to compare against")
args = ap.parse_args()
from vilbert import _native as N  # noqa: E402
if args.lib:
    N.LIB_PATH = os.path.abspath(args.lib)
from vilbert import ops, ops16  # noqa: E402

dev = "cuda:0"
BF16 = torch.bfloat16
g = torch.Generator().manual_seed(4321)


def sha(t):
    t = t.detach().contiguous().reshape(-1)
    raw = t.view(torch.uint8) if t.dtype != torch.uint8 else t
    return hashlib.sha256(raw.cpu().numpy().tobytes()).hexdigest()[:16]


def show(tag, shape, outs):
    torch.cuda.synchronize()
    print("%-26s %-16s %s" % (tag, shape, " ".join("-" if o is None else sha(o) for o in outs)), flush=True)


def rand(*shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def strided(t, pad):
    """the same values as a row-strided view of a wider buffer (pad = 0: the tensor itself)"""
    if pad == 0:
        return t
    buf = torch.full((t.shape[0], t.shape[1] + pad), float("nan"), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def call(name, *a):
    N.check(getattr(N.lib(), name)(N.stream_ptr(), *a), name)


# ---- flat casts
for n in (7, 8, 2055):
    x = rand(n, scale=3.0)
    y = ops16.cast_bf16(x)
    show("cast f32->bf16->f32", n, (y, ops16.cast_f32(y)))

# ---- row casts and loss backwards into the padded bf16 operands
for rows, n in itertools.product((1, 5, 64, 65, 130), (2, 211, 1601)):
    shape = "%d x %d" % (rows, n)
    for pad in (0, (4 - n % 4) % 4 + 4):
        tag = " ld+%d" % pad if pad else ""
        x = strided(rand(rows, n, scale=3.0), pad)
        show("cast_rows" + tag, shape, (ops16.cast_rows_padded(x),))
        show("cast_rows_colsum" + tag, shape, ops16.cast_rows_colsum(ops16.rows_addressable(x)))
        labels = torch.randint(0, n, (rows,), generator=g)
        labels[::3] = -1
        if rows > 1:
            labels[1] = n - 1
        labels = labels.to(dev)
        gl = torch.full((1,), 0.7, device=dev)
        loss, lse, count = ops.xent_fwd(x, labels, -1)
        show("xent fwd" + tag, shape, (loss, lse, count))
        show("xent bwd" + tag, shape, (ops.xent_bwd(gl, x, labels, -1, lse, count),))
        for want_t, want_cs in ((False, False), (True, False), (False, True), (True, True)):
            outs = ops16.xent_bwd16(gl, x, labels, -1, lse, count, want_t, want_colsum=want_cs)
            show("xent16 GT=%d parts=%d%s" % (want_t, want_cs, tag), shape, outs)
            if want_cs:
                show("colsum_parts %d" % outs[2].shape[0], shape, (ops16.colsum_parts(outs[2], n, rand(n)),))
        target = torch.rand(rows, n, generator=g).to(dev)
        for divisor in (float(max(rows, 1)), torch.full((1,), float(rows) + 0.5, device=dev)):
            kind = "host" if isinstance(divisor, float) else "dev"
            loss, lse2, tsum = ops.kl_fwd(x, target, divisor)
            show("kl fwd %s%s" % (kind, tag), shape, (loss, lse2, tsum))
            show("kl bwd %s%s" % (kind, tag), shape, (ops.kl_bwd(gl, x, target, lse2, tsum, divisor),))
            show("kl16 %s%s" % (kind, tag), shape, (ops16.kl_bwd16(gl, x, target, lse2, tsum, divisor),))

# ---- colsum_parts over 3 parts of its own
part = rand(3, 512)
show("colsum_parts 3", "3 x 300", (ops16.colsum_parts(part, 300, rand(300)),))

# ---- weight shadows
for rows, cols in ((64, 64), (128, 192)):
    w = rand(rows, cols)
    for which in ("w16", "wt16", "both"):
        w16 = torch.zeros(rows, cols, dtype=BF16, device=dev)
        wt16 = torch.zeros(cols, rows, dtype=BF16, device=dev)
        call("vb_weight_shadow_bf16", rows, cols, w.data_ptr(), cols, w16.data_ptr() if which != "wt16" else None, cols,
             wt16.data_ptr() if which != "w16" else None, rows)
        show("weight_shadow " + which, "%d x %d" % (rows, cols), (w16, wt16))
SHADOW_REC = np.dtype([("w", "<u8"), ("w16", "<u8"), ("wt16", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("ld16", "<i8"),
                       ("ldt", "<i8"), ("tile0", "<i8")])          # vb_shadow_seg
for shapes in (((64, 128),), ((64, 64), (192, 128), (128, 320))):
    ws = [rand(r, c) for r, c in shapes]
    w16s = [torch.zeros(r, c, dtype=BF16, device=dev) for r, c in shapes]
    wt16s = [torch.zeros(c, r, dtype=BF16, device=dev) for r, c in shapes]
    recs, tile0 = [], 0
    for (r, c), w, a, b in zip(shapes, ws, w16s, wt16s):
        recs.append((w.data_ptr(), a.data_ptr(), b.data_ptr(), r, c, c, r, tile0))
        tile0 += (r // 64) * (c // 64)
    tab = torch.from_numpy(np.array(recs, dtype=SHADOW_REC).view(np.uint8).reshape(-1).copy()).to(dev)
    call("vb_weight_shadow_multi", len(shapes), tab.data_ptr(), tile0)
    show("weight_shadow_multi", "%d segments" % len(shapes), w16s + wt16s)
for n, K in itertools.product((1, 63, 211), (128, 768)):
    w, bias = rand(n, K), rand(n)
    n_pad = ops16.padded(n)
    w16 = torch.zeros(n_pad, K, dtype=BF16, device=dev)
    wt16 = torch.zeros(K, n_pad, dtype=BF16, device=dev)
    bpad = torch.zeros(n_pad, device=dev)
    call("vbh_weight_shadow_ragged", n, K, w.data_ptr(), K, bias.data_ptr(), w16.data_ptr(), wt16.data_ptr(), bpad.data_ptr())
    show("weight_shadow_ragged", "%d x %d" % (n, K), (w16, wt16, bpad))

# ---- column sums of a bf16 matrix
for rows, cols in itertools.product((1, 65, 300), (4, 260)):
    x = rand(rows, cols).to(BF16)
    out = rand(cols)
    ws = torch.zeros(int(N.lib().vb_colsum_bf16_workspace(cols)), device=dev)
    call("vb_colsum_bf16", rows, cols, x.data_ptr(), cols, out.data_ptr(), ws.data_ptr())
    show("colsum_bf16", "%d x %d" % (rows, cols), (out,))

# ---- bf16 row movers
for M, cols in itertools.product((1, 33, 96), (8, 256, 1024)):
    src = strided(rand(50, cols).to(BF16), 16)
    m = torch.full((M,), -1, dtype=torch.int32)
    take = min(50, (M + 1) // 2)
    m[torch.randperm(M, generator=g)[:take]] = torch.randperm(50, generator=g)[:take].to(torch.int32)
    if M > 4:
        m[(m == -1).nonzero()[:2, 0]] = torch.tensor([50, -7], dtype=torch.int32)
    m = m.to(dev)
    c = ops16.gather_rows(src, m)
    inv = torch.empty(50, dtype=torch.int32, device=dev)
    call("vbh_invert_map", 50, M, m.data_ptr(), inv.data_ptr())
    show("gather / invert / scatter", "%d x %d" % (M, cols), (c, inv, ops16.scatter_rows(c, m, 50)))

# ---- pooler ReLU backward, GELU backward multiply
for rows, cols in ((5, 8), (70, 1024)):
    show("relu_bwd16", "%d x %d" % (rows, cols), (ops16.relu_bwd(rand(rows, cols), rand(rows, cols)),))
    show("mul16", "%d x %d" % (rows, cols), (ops16.mul(rand(rows, cols).to(BF16), rand(rows, cols).to(BF16)),))


# ---- the fp32 movers: one BertLayer on a row map (the case of tests/test_last_layer_rows_gpu.py)
def layer_on_a_row_map():
    import vilbert.autograd_ops as AO
    from oracle import synth
    from vilbert import layers
    from vilbert.vilbert import BertConfig, BertLayer
    B, S, H = 3, 5, 32
    torch.manual_seed(7)
    layer = BertLayer(BertConfig.from_dict(synth.tiny_config(hidden_size=H, num_attention_heads=1, intermediate_size=40)))
    layer = layer.to(dev).train()
    for p in layer.parameters():
        p.data.add_(torch.randn_like(p) * 0.05)
    x = torch.randn(B, S, H, device=dev).requires_grad_(True)
    mask = torch.zeros(B, 1, 1, S, device=dev)
    mask[1, 0, 0, 4] = -10000.0
    rows = torch.tensor([0, 5, 10, 7, -1, 13, 2], dtype=torch.int32, device=dev)
    w = torch.randn(rows.numel(), H, device=dev) * (rows >= 0).unsqueeze(1)
    AO._seed_counter = itertools.count(1)
    y = layers.self_layer(layer, x, mask, 0.1, 0.1, 0.1, rows)
    (y * w).sum().backward()
    show("layer on a row map", "3 x 5 x 32", [y, x.grad] + [p.grad for _, p in sorted(layer.named_parameters())])


layer_on_a_row_map()

# ---- task losses
for rows, n in itertools.product((1, 5, 70), (2, 3, 211, 3129)):
    shape = "%d x %d" % (rows, n)
    x, t = rand(rows, n, scale=3.0), torch.rand(rows, n, generator=g).to(dev)
    show("bce fwd / bwd", shape, (ops.bce_fwd(x, t), ops.bce_bwd(torch.full((1,), 0.7, device=dev), x, t)))
    show("argmax_pick", shape, ops.argmax_pick(x, t, want_dense=True))

# ---- NCE region loss
for (B, R, dim, n_neg) in ((2, 3, 64, 4), (4, 9, 2048, 16)):
    rows = B * R
    predict, table = rand(rows, dim), rand(rows, dim)
    pos = torch.arange(rows, device=dev)
    neg = ops.nce_negatives(pos, B, R, n_neg // 2, n_neg - n_neg // 2, 11)
    valid = (torch.arange(rows) % 4 != 1).to(dev)
    count = valid.sum().to(torch.float32).reshape(1)
    loss, dsave = ops.nce_fwd(predict, table, pos, neg, valid, count)
    show("nce fwd / bwd", "%d x %d, %d neg" % (rows, dim, n_neg),
         (neg, loss, dsave, ops.nce_bwd(torch.full((1,), 0.7, device=dev), dsave, valid, count)))

# ---- skinny linear
for rows, K, n, p in itertools.product((1, 70), (128, 1024), (1, 3), (0.0, 0.1)):
    shape = "%d x %d -> %d p=%.1f" % (rows, K, n, p)
    x, w, b, dy = rand(rows, K).to(BF16), rand(n, K), rand(n), rand(rows, n)
    dws, dbs = ops16.skinny_bwd_weight(dy, x, n, True, drop_p=p, seed=5)
    show("skinny fwd / dgrad / wgrad", shape, (ops16.skinny_fwd(x, w, b, drop_p=p, seed=5),
                                                ops16.skinny_bwd_input(dy, w, drop_p=p, seed=5), dws[0], dbs[0]))
