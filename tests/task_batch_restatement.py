"""numpy restatement of the device-side fine-tuning batch builder (csrc/task_batch.hip; include/vilbert_hip_task_inputs.h): THE
spec of its kernels, in their order of operations. Every fp32 operation is one IEEE operation rounded to nearest (numpy on fp32
arrays and scalars does exactly that; nothing is fused), the column sum is an explicit loop over the rows in row order, and the
divides stay in fp32. tests/test_task_batch.py holds it to outputs recorded from the reference's own datasets
(tests/golden/task_batch.npz) and to ``np.sum(x, axis=0) / n``; tests/test_task_batch_gpu.py holds the kernels to it bit for bit.
"""
import numpy as np

f32 = np.float32
ONE = f32(1.0)


def span(lo, hi, total_rows, mean_rows, max_regions):
    """csrc/task_rows.h: (start, rows, mean, kept) of a sample whose offsets words are lo, hi; mean_rows None = all rows."""
    n = max(int(total_rows), 0)
    start = min(max(int(lo), 0), n)
    rows = min(max(int(hi) - start, 0), n - start)
    mean = rows if mean_rows is None else min(max(int(mean_rows), 0), rows)
    return start, rows, mean, min(rows + 1, max(int(max_regions), 1))


def mean_row(x):
    """fp32 sum of the rows of x [n, F] in row order, divided in fp32 by float32(n); zeros for n == 0."""
    x = np.asarray(x, dtype=f32)
    s = np.zeros(x.shape[1], dtype=f32)
    for row in x:
        s = s + row                          # float32 + float32, one rounding per row
    if x.shape[0] == 0:
        return s
    return s / f32(x.shape[0])


def iou_px(a, g):
    """The reference's iou() (+ 1 pixel convention) of the pixel boxes a [n, 4] against one box g [4], fp32 throughout."""
    a, g = np.asarray(a, dtype=f32).reshape(-1, 4), np.asarray(g, dtype=f32)
    g_area = ((g[2] - g[0]) + ONE) * ((g[3] - g[1]) + ONE)
    a_area = ((a[:, 2] - a[:, 0]) + ONE) * ((a[:, 3] - a[:, 1]) + ONE)
    iw = (np.minimum(a[:, 2], g[2]) - np.maximum(a[:, 0], g[0])) + ONE
    ih = (np.minimum(a[:, 3], g[3]) - np.maximum(a[:, 1], g[1])) + ONE
    iw = np.where(iw < 0, f32(0), iw)
    ih = np.where(ih < 0, f32(0), ih)
    inter = iw * ih
    with np.errstate(divide="ignore", invalid="ignore"):
        return (inter / ((a_area + g_area) - inter)).astype(f32)


def finish_task_batch(packed, max_regions, ref_box=None, iou_floor=0.0):
    """packed: dict of numpy arrays feat [N, F], boxes [N, 4], offsets [B + 1], image_wh [B, 2], mean_rows [B] or None.
    Returns (features [B, R, F], spatials [B, R, 5], image_mask [B, R] int64[, target [B, R, 1]])."""
    feat, boxes = np.asarray(packed["feat"], dtype=f32), np.asarray(packed["boxes"], dtype=f32).reshape(-1, 4)
    offsets, wh = np.asarray(packed["offsets"]), np.asarray(packed["image_wh"])
    mean_rows = packed.get("mean_rows")
    B, R, F, N = len(offsets) - 1, int(max_regions), feat.shape[1], feat.shape[0]
    out_feat = np.zeros((B, R, F), dtype=f32)
    out_sp = np.zeros((B, R, 5), dtype=f32)
    out_mask = np.zeros((B, R), dtype=np.int64)
    out_iou = np.zeros((B, R, 1), dtype=f32) if ref_box is not None else None
    for b in range(B):
        start, rows, mean, kept = span(offsets[b], offsets[b + 1], N, None if mean_rows is None else mean_rows[b], R)
        out_feat[b, 0] = mean_row(feat[start:start + mean])
        out_feat[b, 1:kept] = feat[start:start + kept - 1]
        W, H = int(wh[b, 0]), int(wh[b, 1])
        w, h, area = f32(W), f32(H), f32(W * H)            # the exact product rounded to fp32 once
        px = boxes[start:start + kept - 1]
        out_sp[b, 0] = (0, 0, 1, 1, 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            out_sp[b, 1:kept, 0] = px[:, 0] / w
            out_sp[b, 1:kept, 1] = px[:, 1] / h
            out_sp[b, 1:kept, 2] = px[:, 2] / w
            out_sp[b, 1:kept, 3] = px[:, 3] / h
            out_sp[b, 1:kept, 4] = ((px[:, 3] - px[:, 1]) * (px[:, 2] - px[:, 0])) / area
        out_mask[b, :kept] = 1
        if out_iou is not None:
            anchors = np.concatenate([np.array([[0, 0, w, h]], dtype=f32), px], axis=0)
            t = iou_px(anchors, np.asarray(ref_box, dtype=f32)[b])
            out_iou[b, :kept, 0] = np.where(t < f32(iou_floor), f32(0), t)
    return (out_feat, out_sp, out_mask) + (() if out_iou is None else (out_iou,))


def dense_target(labels, scores, num_labels, ldt=None, out=None):
    """labels [B, K] int32 padded with -1, scores [B, K] fp32 -> [B, num_labels] fp32 (row stride ldt: the columns beyond
    num_labels of `out` keep what they held): zero, or the score of the LAST k whose label is the column."""
    labels, scores = np.asarray(labels), np.asarray(scores, dtype=f32)
    B, K = labels.shape
    ldt = int(num_labels) if ldt is None else int(ldt)
    target = np.zeros((B, ldt), dtype=f32) if out is None else np.array(out, dtype=f32).reshape(B, ldt)
    target[:, :num_labels] = 0
    for b in range(B):
        for k in range(K):
            if 0 <= labels[b, k] < num_labels:
                target[b, labels[b, k]] = scores[b, k]
    return target


def make_packed(n_rows, feat_dim, seed, mean_rows=None, big_image=None):
    """A synthetic packed batch: full-mantissa features, boxes inside images of 200 .. 1000 pixels a side (sample `big_image`
    gets 5000 x 4000: W * H beyond 2^24)."""
    rng = np.random.default_rng(seed)
    B, N = len(n_rows), int(sum(n_rows))
    feat = (rng.standard_normal((N, feat_dim)) * np.exp(rng.uniform(-3, 3, (N, 1)))).astype(f32)
    wh = rng.integers(200, 1000, (B, 2)).astype(np.int32)
    if big_image is not None:
        wh[big_image] = (5000, 4000)
    offsets = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int64)
    boxes = np.zeros((N, 4), dtype=f32)
    for b in range(B):
        n = n_rows[b]
        lo = rng.uniform(0, 0.7, (n, 2)) * wh[b]
        hi = lo + rng.uniform(0.01, 0.3, (n, 2)) * wh[b]
        boxes[offsets[b]:offsets[b + 1]] = np.concatenate([lo, hi], axis=1).astype(f32)
    return dict(feat=feat, boxes=boxes, offsets=offsets, image_wh=wh,
                mean_rows=None if mean_rows is None else np.asarray(mean_rows, dtype=np.int32))
