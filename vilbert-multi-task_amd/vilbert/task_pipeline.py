"""Device-side batch builder of the fine-tuning tasks (``vilbert.input_pipeline`` is the pre-training one).

The reference builds every fine-tuning sample on the host (vilbert/datasets/_image_features_reader.py:144-176: mean-region row
and a 5-number box per region in numpy; vqa_dataset.py:275-310, refer_expression_dataset.py:241-296: ``np.zeros((max_region_num,
2048))`` in float64, a copy into it, back to float32, a dense ``[num_labels]`` answer target or the region IoU against the
reference box) and the collate stacks the padded samples into ``[B, max_region_num, 2048]``. Detector outputs have 10 - 100
boxes, so at 101 regions much of what is built, stacked and copied is zeros.

Here a source hands over PACKED region data - the regions of all samples back to back (``pack_task_samples``: host-side
concatenation only), pixel boxes, image sizes, sparse answers or a reference box - and the device writes the model's inputs
(csrc/task_batch.hip, ``vbd_task_finish_batch`` + ``vbd_dense_target``; include/vilbert_hip_task_inputs.h states the arithmetic,
held bit for bit to the reference's own). ``TaskBatchPipeline`` yields the tuple the reference's datasets collate to:
    (features, spatials, image_mask, question, target, input_mask, segment_ids, co_attention_mask, question_id)

Half-width features (opt-in): ``pack_task_samples(..., dtype=np.float16)`` packs float16 region features,
``TaskBatchPipeline(..., wire_dtype=torch.float16)`` sends them as they are and the device widens them while it builds the batch
(csrc/task_batch.hip, ``vbw_task_finish_batch``; include/vilbert_hip_wire.h) - the bits of the default builder on the widened
arrays, or with ``feature_dtype=torch.bfloat16`` those bits rounded to bf16 for the bf16 stream.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .staging import StagedPipeline, out_kind

PACKED_FIELDS = ("feat", "boxes", "offsets", "image_wh", "mean_rows")
TOKEN_FIELDS = ("question", "input_mask", "segment_ids")
_DTYPES = dict(feat=torch.float32, boxes=torch.float32, offsets=torch.int64, image_wh=torch.int32, mean_rows=torch.int32,
               question=torch.int64, input_mask=torch.int64, segment_ids=torch.int64, question_id=torch.int64,
               labels=torch.int32, scores=torch.float32, ref_box=torch.float32)


def raw_item(item):
    """One raw sample from the reference's LMDB record (``features``, ``boxes``, ``image_w``, ``image_h``): the reshapes of
    the reference's reader (_image_features_reader.py:144-145) and nothing else - no mean row, no box arithmetic."""
    return dict(feat=np.asarray(item["features"], dtype=np.float32).reshape(-1, 2048),
                boxes=np.asarray(item["boxes"], dtype=np.float32).reshape(-1, 4),
                image_w=int(item["image_w"]), image_h=int(item["image_h"]))


def pack_task_samples(samples, mean_rows=None, dtype=np.float32):
    """samples: raw samples (``raw_item``), one per IMAGE - a multi-image task (NLVR2 pairs, retrieval options) packs each
    image as its own entry. Returns numpy arrays: feat [N, F] and boxes [N, 4] (the samples back to back), offsets [B + 1]
    int64, image_wh [B, 2] int32, mean_rows [B] int32 (the leading rows of a sample that enter its mean; default: all of them -
    the refer-expression training split appends ground-truth rows that do not). Host-side concatenation only.
    dtype=np.float16: for a store that keeps float16 features - every sample's features must BE float16 (ValueError
    otherwise: nothing is narrowed here) and feat is packed as float16, for ``wire_dtype=torch.float16``."""
    if len(samples) == 0:
        raise ValueError("no samples to pack")
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.float32), np.dtype(np.float16)):
        raise ValueError("dtype must be numpy.float32 or numpy.float16, got %r" % (dtype,))
    if dtype == np.float16:
        for i, s in enumerate(samples):
            if np.asarray(s["feat"]).dtype != np.float16:
                raise ValueError("sample %d: dtype=float16 takes float16 features, got %s (the packer never narrows)"
                                 % (i, np.asarray(s["feat"]).dtype))
    feats = [np.asarray(s["feat"], dtype=dtype) for s in samples]
    boxes = [np.asarray(s["boxes"], dtype=np.float32).reshape(-1, 4) for s in samples]
    F = feats[0].shape[-1]
    for i, (f, bx) in enumerate(zip(feats, boxes)):
        if f.ndim != 2 or f.shape[1] != F:
            raise ValueError("sample %d: features of shape %s in a batch of width %d" % (i, f.shape, F))
        if f.shape[0] == 0:
            raise ValueError("sample %d has no regions" % i)
        if bx.shape[0] != f.shape[0]:
            raise ValueError("sample %d: %d feature rows, %d boxes" % (i, f.shape[0], bx.shape[0]))
        if int(samples[i]["image_w"]) <= 0 or int(samples[i]["image_h"]) <= 0:
            raise ValueError("sample %d: image size %r x %r" % (i, samples[i]["image_w"], samples[i]["image_h"]))
    rows = np.array([f.shape[0] for f in feats], dtype=np.int64)
    if mean_rows is None:
        mean = rows.astype(np.int32)
    else:
        mean = np.asarray(mean_rows, dtype=np.int64)
        if mean.shape != rows.shape or (mean < 1).any() or (mean > rows).any():
            raise ValueError("mean_rows must hold one count in [1, rows] per sample, got %r for %r rows" % (mean_rows, rows))
        mean = mean.astype(np.int32)
    return dict(feat=np.concatenate(feats, axis=0), boxes=np.concatenate(boxes, axis=0),
                offsets=np.concatenate([[0], np.cumsum(rows)]).astype(np.int64),
                image_wh=np.array([(int(s["image_w"]), int(s["image_h"])) for s in samples], dtype=np.int32), mean_rows=mean)


def _dev(t, name, dtype, shape):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s: expected a tensor on a HIP device - the MI355X-native path has no CPU fallback" % name)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise RuntimeError("%s: expected a contiguous %s tensor of shape %s, got %s %s"
                           % (name, dtype, list(shape), t.dtype, tuple(t.shape)))
    return t.data_ptr()


def finish_task_batch(packed_dev, max_regions, ref_box=None, iou_floor=0.0, out_dtype=torch.float32):
    """packed_dev: dict of DEVICE tensors named as ``pack_task_samples`` names them (mean_rows may be missing or None: all
    rows enter the mean). Returns (features [B, R, F], spatials [B, R, 5], image_mask [B, R] int64) and, with ref_box [B, 4]
    (pixel x1, y1, x2, y2), the region-IoU target [B, R, 1] (values below iou_floor become 0). One native launch pair on the
    current stream; every element of the outputs is written by it, no torch arithmetic.
    A float16 feat is widened by the same pass: the bits the fp32 builder gives on the widened rows, or with
    out_dtype=torch.bfloat16 (float16 feat only) those bits rounded to bf16."""
    feat, offsets = packed_dev["feat"], packed_dev["offsets"]
    if not isinstance(feat, torch.Tensor) or feat.dim() != 2 or not isinstance(offsets, torch.Tensor) or offsets.dim() != 1 \
            or offsets.shape[0] < 1:
        raise RuntimeError("feat must be [rows, feat_dim] and offsets [batch + 1]")
    (n, F), B, R, dev = feat.shape, offsets.shape[0] - 1, int(max_regions), feat.device
    half = feat.dtype == torch.float16
    kind = out_kind(out_dtype, half, "finish_task_batch")
    a = N.WireTaskBatch() if half else N.TaskBatchArgs()
    a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.total_rows = B, R, F, float(iou_floor), n
    if half:
        a.out_kind = kind
    a.feat = _dev(feat, "feat", torch.float16 if half else torch.float32, (n, F))
    a.boxes = _dev(packed_dev["boxes"], "boxes", torch.float32, (n, 4))
    a.offsets = _dev(offsets, "offsets", torch.int64, (B + 1,))
    a.image_wh = _dev(packed_dev["image_wh"], "image_wh", torch.int32, (B, 2))
    if packed_dev.get("mean_rows") is not None:
        a.mean_rows = _dev(packed_dev["mean_rows"], "mean_rows", torch.int32, (B,))
    out_feat = torch.empty(B, max(R, 0), F, dtype=out_dtype, device=dev)
    out_sp = torch.empty(B, max(R, 0), 5, dtype=torch.float32, device=dev)
    out_mask = torch.empty(B, max(R, 0), dtype=torch.int64, device=dev)
    a.out_feat, a.out_spatials, a.out_mask = out_feat.data_ptr(), out_sp.data_ptr(), out_mask.data_ptr()
    out = (out_feat, out_sp, out_mask)
    if ref_box is not None:
        a.ref_box = _dev(ref_box, "ref_box", torch.float32, (B, 4))
        out_iou = torch.empty(B, max(R, 0), 1, dtype=torch.float32, device=dev)
        a.out_iou = out_iou.data_ptr()
        out += (out_iou,)
    if half:
        N.check(N.lib().vbw_task_finish_batch(N.stream_ptr(), ctypes.byref(a)), "vbw_task_finish_batch")
    else:
        N.check(N.lib().vbd_task_finish_batch(N.stream_ptr(), ctypes.byref(a)), "vbd_task_finish_batch")
    return out


def dense_target(labels, scores, num_labels):
    """labels [B, K] int32 (padded with -1), scores [B, K] fp32, both on the device -> the dense soft-label target
    [B, num_labels] of the VQA-style heads: zero, or the score of the last k whose label is the column. One native launch
    writes every element; nothing is cleared first."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 2:
        raise RuntimeError("labels must be [batch, K]")
    B, K = labels.shape
    out = torch.empty(B, max(int(num_labels), 0), dtype=torch.float32, device=labels.device)
    N.check(N.lib().vbd_dense_target(N.stream_ptr(), B, int(num_labels), K, _dev(labels, "labels", torch.int32, (B, K)),
                                     _dev(scores, "scores", torch.float32, (B, K)), out.data_ptr(), int(num_labels)),
            "vbd_dense_target")
    return out


class TaskBatchPipeline(StagedPipeline):
    """Iterate over ``source`` - an iterable of batches, each a dict of numpy arrays: the five arrays of
    ``pack_task_samples``, the token arrays ``question``, ``input_mask``, ``segment_ids`` [B, T], ``question_id`` [B] and what
    the target needs - and yield finished device batches in the reference datasets' tuple order
        (features, spatials, image_mask, question, target, input_mask, segment_ids, co_attention_mask, question_id).

    target=None               the batch's own ``target`` array is copied as it is, in its own dtype (tasks whose target is a label)
    target=("dense", L)       ``labels`` / ``scores`` [B, K] (int32 padded with -1 / fp32) become the dense [B, L] target
    target=("iou", floor)     ``ref_box`` [B, 4] (pixel x1, y1, x2, y2) becomes the region-IoU target [B, R, 1]

    Batch i + 1 is staged on a dedicated stream right after the caller has enqueued step i (``StagedPipeline``: double
    buffered, two staging modes). The packed arrays change length from batch to batch: a slot's buffers are sized by
    CAPACITY (first dimension, grow only) and a batch uses a leading view of them. The token tensors are copied as they are
    and alias the slot's device buffers: they stay valid until the caller asks for batch i + depth - 1. co_attention_mask
    is one cached zero tensor [B, R, T] (the reference builds a fresh one per sample; nothing writes to it).

    wire_dtype=torch.float16: ``feat`` must be a float16 array (``pack_task_samples(..., dtype=np.float16)``; anything else
    raises ValueError - the pipeline never narrows), crosses the bus as it is and is widened on the device: the bits of the
    default pipeline fed the widened array. feature_dtype=torch.bfloat16 (with the float16 wire only) yields the features
    rounded to bf16."""

    dtypes, wire_fields = _DTYPES, ("feat",)

    def __init__(self, source, device, max_regions, target=None, depth=2, staging=None, wire_dtype=None,
                 feature_dtype=torch.float32):
        StagedPipeline.__init__(self, source, device, depth, staging, wire_dtype, feature_dtype)
        self.max_regions = int(max_regions)
        if target is not None and (len(target) != 2 or target[0] not in ("dense", "iou")):
            raise ValueError("target must be None, ('dense', num_labels) or ('iou', floor), got %r" % (target,))
        self.target = target
        # a target the source supplies keeps its own dtype (int64 labels for cross-entropy, fp32 soft labels)
        extra = {None: ("target",), "dense": ("labels", "scores"), "iou": ("ref_box",)}[target[0] if target else None]
        self.fields = PACKED_FIELDS + TOKEN_FIELDS + ("question_id",) + extra
        self._co_attention = {}

    def arrays(self, batch):
        return batch, ()

    def _zeros(self, B, T):
        t = self._co_attention.get((B, T))
        if t is None:
            t = self._co_attention[(B, T)] = torch.zeros(B, self.max_regions, T, dtype=torch.float32, device=self.device)
        return t

    def finish(self, slot):
        v = slot.views
        kind = self.target[0] if self.target else None
        out = finish_task_batch(v, self.max_regions, ref_box=v["ref_box"] if kind == "iou" else None,
                                iou_floor=float(self.target[1]) if kind == "iou" else 0.0, out_dtype=self.feature_dtype)
        if kind == "dense":
            target = dense_target(v["labels"], v["scores"], int(self.target[1]))
        else:
            target = out[3] if kind == "iou" else v["target"]
        B, T = v["question"].shape
        return (out[0], out[1], out[2], v["question"], target, v["input_mask"], v["segment_ids"], self._zeros(B, T),
                v["question_id"])
