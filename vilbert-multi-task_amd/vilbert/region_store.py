"""Device-resident region store: fine-tuning batches by image index (opt-in; ``vilbert.task_pipeline`` is the default).

``TaskBatchPipeline`` packs the regions of every batch on the host and copies them to the device - at the VQA shape tens of MB
per step. The detector's regions of a fine-tuning dataset fit on one device (a region is 2048 float16 values, 4 KB; 31 k images
of 100 boxes are about 13 GB), so they can be copied there ONCE: ``RegionStore`` holds them image after image, and a batch is
then named by one image id per sample. The device gathers each sample's rows itself (csrc/region_store.hip,
``vbr_store_finish_batch``; include/vilbert_hip_store.h) with the kernels of the packed builder, so what comes out is what
``finish_task_batch`` gives for ``pack_task_samples`` of the same images, bit for bit. An image that a task shows several times
(VCR's four answers, retrieval's options, NLVR2's pairs) is a repeated id.

    store = RegionStore.from_samples(samples, "cuda:0")          # once per dataset; samples: ``raw_item`` records, float16
    for batch in StoreBatchPipeline(source, store, 101, target=("dense", 3129)):
        ...                                                      # source yields image_ids [B] + the token arrays
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .staging import out_kind
from .task_pipeline import _DTYPES, TOKEN_FIELDS, TaskBatchPipeline, _dev, dense_target, pack_task_samples

_NUMPY_DTYPES = {torch.float16: np.dtype(np.float16), torch.float32: np.dtype(np.float32)}


class RegionStore(object):
    """The regions of up to ``capacity_images`` images, ``capacity_rows`` rows in all, on ``device``: feat [rows, feat_dim]
    (``dtype``: torch.float16 or torch.float32), boxes [rows, 4], image_offsets [images + 1] int64, image_wh [images, 2] int32,
    mean_rows [images] int32. The five arrays are allocated once, at capacity, by the first ``add`` (the constructor touches no
    device); they never grow - a store is tens of GB, and a silent second copy of it is not a thing to do behind a caller's
    back. ``with_mean_rows``: the batches honour each image's count of leading rows that enter its mean (the refer-expression
    training split appends ground-truth rows that do not); without it every row of an image does, and ``add`` refuses a pack
    that says otherwise."""

    def __init__(self, device, capacity_rows, capacity_images, feat_dim=2048, dtype=torch.float16, with_mean_rows=False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RegionStore: expected a HIP device, got %r - the MI355X-native path has no CPU fallback" % (device,))
        if dtype not in _NUMPY_DTYPES:
            raise ValueError("RegionStore: dtype must be torch.float16 or torch.float32, got %r" % (dtype,))
        group = 8 if dtype == torch.float16 else 4
        if int(capacity_rows) < 0 or int(capacity_images) < 0 or int(feat_dim) <= 0 or int(feat_dim) % group != 0:
            raise ValueError("RegionStore: capacities must not be negative and feat_dim a positive multiple of %d, got %r rows, "
                             "%r images, feat_dim %r" % (group, capacity_rows, capacity_images, feat_dim))
        self.capacity_rows, self.capacity_images, self.feat_dim = int(capacity_rows), int(capacity_images), int(feat_dim)
        self.dtype, self.with_mean_rows = dtype, bool(with_mean_rows)
        self.total_rows = self.num_images = 0
        self.feat = self.boxes = self.image_offsets = self.image_wh = self.mean_rows = None

    @property
    def nbytes(self):
        """Device bytes of the five arrays (at capacity, whatever is filled)."""
        rows, images = self.capacity_rows, self.capacity_images
        return rows * self.feat_dim * _NUMPY_DTYPES[self.dtype].itemsize + rows * 16 + (images + 1) * 8 + images * 8 + images * 4

    def _allocate(self):
        if self.feat is None:
            rows, images, dev = self.capacity_rows, self.capacity_images, self.device
            self.feat = torch.empty(rows, self.feat_dim, dtype=self.dtype, device=dev)
            self.boxes = torch.empty(rows, 4, dtype=torch.float32, device=dev)
            self.image_offsets = torch.zeros(images + 1, dtype=torch.int64, device=dev)
            self.image_wh = torch.empty(images, 2, dtype=torch.int32, device=dev)
            self.mean_rows = torch.empty(images, dtype=torch.int32, device=dev)

    def add(self, packed):
        """Append the images of ``packed`` (a dict from ``pack_task_samples``, feat in the store's own dtype: nothing is
        narrowed or widened here) with plain tensor copies; its offsets are rebased on the host by the current row count.
        Returns the ``range`` of image ids it assigned. A chunk beyond either capacity raises ValueError and changes nothing."""
        feat, offsets = np.asarray(packed["feat"]), np.asarray(packed["offsets"], dtype=np.int64)
        if feat.dtype != _NUMPY_DTYPES[self.dtype]:
            raise ValueError("RegionStore.add: a %s store takes %s features, got %s (the store never narrows or widens)"
                             % (self.dtype, _NUMPY_DTYPES[self.dtype], feat.dtype))
        if feat.ndim != 2 or feat.shape[1] != self.feat_dim:
            raise ValueError("RegionStore.add: features of shape %s in a store of width %d" % (feat.shape, self.feat_dim))
        n, k = feat.shape[0], offsets.shape[0] - 1
        boxes = np.asarray(packed["boxes"], dtype=np.float32).reshape(-1, 4)
        wh, mean = np.asarray(packed["image_wh"], dtype=np.int32), np.asarray(packed["mean_rows"], dtype=np.int32)
        if k < 1 or offsets[0] != 0 or offsets[-1] != n or (np.diff(offsets) < 1).any() or boxes.shape[0] != n \
                or wh.shape != (k, 2) or mean.shape != (k,):
            raise ValueError("RegionStore.add: not a pack of pack_task_samples (%d rows, offsets %r ...)" % (n, offsets[:4].tolist()))
        if not self.with_mean_rows and not np.array_equal(mean, np.diff(offsets)):
            raise ValueError("RegionStore.add: the pack counts fewer rows into a mean than an image has; build the store with "
                             "with_mean_rows=True")
        if self.total_rows + n > self.capacity_rows or self.num_images + k > self.capacity_images:
            raise ValueError("RegionStore.add: %d + %d rows of %d, %d + %d images of %d: beyond the store's capacity (it does not "
                             "grow)" % (self.total_rows, n, self.capacity_rows, self.num_images, k, self.capacity_images))
        self._allocate()
        r0, i0 = self.total_rows, self.num_images
        self.feat[r0:r0 + n].copy_(torch.from_numpy(np.ascontiguousarray(feat)))
        self.boxes[r0:r0 + n].copy_(torch.from_numpy(np.ascontiguousarray(boxes)))
        self.image_offsets[i0 + 1:i0 + 1 + k].copy_(torch.from_numpy(offsets[1:] + r0))
        self.image_wh[i0:i0 + k].copy_(torch.from_numpy(np.ascontiguousarray(wh)))
        self.mean_rows[i0:i0 + k].copy_(torch.from_numpy(np.ascontiguousarray(mean)))
        self.total_rows, self.num_images = r0 + n, i0 + k
        return range(i0, i0 + k)

    @classmethod
    def from_samples(cls, samples, device, dtype=torch.float16, chunk=1024, mean_rows=None):
        """A store of exactly the size of ``samples`` (a sequence of ``raw_item`` records, one per image), added ``chunk``
        images at a time: the host never holds a second full copy. Image i of the store is samples[i]."""
        if dtype not in _NUMPY_DTYPES:
            raise ValueError("RegionStore: dtype must be torch.float16 or torch.float32, got %r" % (dtype,))
        if len(samples) == 0:
            raise ValueError("no samples to store")
        rows = sum(int(np.shape(s["feat"])[0]) for s in samples)
        store = cls(device, rows, len(samples), feat_dim=int(np.shape(samples[0]["feat"])[-1]), dtype=dtype,
                    with_mean_rows=mean_rows is not None)
        step = max(int(chunk), 1)
        for i in range(0, len(samples), step):
            store.add(pack_task_samples(samples[i:i + step], mean_rows=None if mean_rows is None else mean_rows[i:i + step],
                                        dtype=_NUMPY_DTYPES[dtype]))
        return store

    def host_ids(self, image_ids):
        """``image_ids`` from the host (a sequence or numpy array of integers in [0, num_images); ValueError otherwise) as a
        contiguous int64 array."""
        ids = np.asarray(image_ids)
        if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
            raise ValueError("image_ids must be a 1-D sequence of integers, got %s %s" % (ids.dtype, ids.shape))
        if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= self.num_images):
            raise ValueError("image_ids must lie in [0, %d), got %d .. %d" % (self.num_images, int(ids.min()), int(ids.max())))
        return np.ascontiguousarray(ids, dtype=np.int64)

    def batch(self, image_ids, max_regions, ref_box=None, iou_floor=0.0, out_dtype=torch.float32):
        """The padded inputs of the batch whose sample b shows image image_ids[b]: what ``finish_task_batch`` returns for
        ``pack_task_samples`` of those images - (features [B, R, F], spatials [B, R, 5], image_mask [B, R] int64) and, with
        ref_box [B, 4] (a device tensor, one box per SAMPLE), the region-IoU target [B, R, 1]. One native launch pair on the
        current stream, no torch arithmetic; out_dtype=torch.bfloat16 needs a float16 store.
        image_ids from the host are validated (``host_ids``) and uploaded. A device int64 tensor is used as it is - nothing is
        read back, so the call can be captured in a graph and replayed on new ids - and the device rule holds: an id outside
        [0, num_images) reads nothing and gives a sample of padding only, image_mask row all 0."""
        half = self.dtype == torch.float16
        kind = out_kind(out_dtype, half, "RegionStore.batch")
        if not isinstance(image_ids, torch.Tensor):
            image_ids = torch.from_numpy(self.host_ids(image_ids)).to(self.device)
        if image_ids.dim() != 1:
            raise RuntimeError("image_ids must be [batch]")
        self._allocate()
        B, R, F, dev = image_ids.shape[0], int(max_regions), self.feat_dim, self.device
        a = N.StoreBatchArgs()
        a.batch, a.max_regions, a.feat_dim, a.iou_floor = B, R, F, float(iou_floor)
        a.feat_kind, a.out_kind = N.STORE_FEAT_KINDS[self.dtype], kind
        a.total_rows, a.num_images = self.total_rows, self.num_images          # the filled part only
        a.feat, a.boxes, a.image_offsets = self.feat.data_ptr(), self.boxes.data_ptr(), self.image_offsets.data_ptr()
        a.image_wh = self.image_wh.data_ptr()
        if self.with_mean_rows:
            a.mean_rows = self.mean_rows.data_ptr()
        a.image_ids = _dev(image_ids, "image_ids", torch.int64, (B,))
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
        if B > 0:                                                   # (an empty tensor has no address to hand over)
            N.check(N.lib().vbr_store_finish_batch(N.stream_ptr(), ctypes.byref(a)), "vbr_store_finish_batch")
        return out


class StoreBatchPipeline(TaskBatchPipeline):
    """``TaskBatchPipeline`` over a ``RegionStore``: the batches of ``source`` carry ``image_ids`` [B] (integers in
    [0, store.num_images); ValueError otherwise) where that pipeline's carry the five packed arrays, and otherwise the same
    arrays - the token arrays ``question``, ``input_mask``, ``segment_ids`` [B, T], ``question_id`` [B] and what the target needs
    (``target`` / ``labels`` + ``scores`` / ``ref_box``). It yields the same 9-tuple with the same ``target`` options, staged by
    the same double-buffered loop; of the regions nothing travels: a float16 store gives the float16-wire bits (and, with
    feature_dtype=torch.bfloat16, the bf16 feature block), an fp32 store the default pipeline's."""

    dtypes, wire_fields = dict(_DTYPES, image_ids=torch.int64), ()

    def __init__(self, source, store, max_regions, target=None, depth=2, staging=None, feature_dtype=torch.float32):
        TaskBatchPipeline.__init__(self, source, store.device, max_regions, target=target, depth=depth, staging=staging,
                                   wire_dtype=torch.float16 if store.dtype == torch.float16 else None,
                                   feature_dtype=feature_dtype)
        self.store = store
        self.fields = ("image_ids",) + self.fields[self.fields.index(TOKEN_FIELDS[0]):]

    def arrays(self, batch):
        return dict(batch, image_ids=self.store.host_ids(batch["image_ids"])), ()

    def finish(self, slot):
        v = slot.views
        kind = self.target[0] if self.target else None
        out = self.store.batch(v["image_ids"], self.max_regions, ref_box=v["ref_box"] if kind == "iou" else None,
                               iou_floor=float(self.target[1]) if kind == "iou" else 0.0, out_dtype=self.feature_dtype)
        if kind == "dense":
            target = dense_target(v["labels"], v["scores"], int(self.target[1]))
        else:
            target = out[3] if kind == "iou" else v["target"]
        B, T = v["question"].shape
        return (out[0], out[1], out[2], v["question"], target, v["input_mask"], v["segment_ids"], self._zeros(B, T),
                v["question_id"])
