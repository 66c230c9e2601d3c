"""Device-side input pipeline of the pre-training step.

The reference finishes every batch on the host (numpy: global mean-region row, concatenations -
vilbert/datasets/concept_cap_dataset.py:241-282), converts to torch, copies ten tensors with ``.cuda()``
inside the step and edits the labels for objective 1 with a few torch ops (train_concap.py:529-540). At
batch 512 that is ~270 MB of numpy concatenation per step on one core - comparable to the GPU step itself.

Here the RAW worker arrays are staged through pinned host buffers, copied on a dedicated HIP stream while
the previous step computes (double buffered), and finished by one native pass (csrc/batch.hip,
``vb_concap_finish_batch``). ``DeviceBatchPipeline`` yields exactly the tuple the reference training loop
unpacks after its own ``.cuda()`` calls and label edit:
    (input_ids, input_mask, segment_ids, lm_label_ids, is_next, image_feat, image_loc, image_target,
     image_label, image_mask)

Dynamic masking (opt-in, ``DeviceBatchPipeline(..., masking=Masking(...))``): the source keeps UNMASKED samples
(``RAW_UNMASKED_FIELDS``: the pairwise IoU of the boxes travels in the slot of ``masked_label``) and which tokens and
regions a step predicts is drawn on the device by ``mask_batch`` (csrc/mask_batch.hip, ``vbi_concap_mask_batch`` +
``vbi_zero_rows``) right before ``finish_batch``. The per-site rule and the probabilities are those of the reference's
``random_word`` / ``random_region``; the draws come from the library's counter-based hash, NOT from Python's ``random``
stream, so the masks of a run differ from the reference's while having the same distribution.

Half-width features (opt-in, ``DeviceBatchPipeline(..., wire_dtype=torch.float16)``): a source that keeps the detector's
post-ReLU activations (and the region targets) as float16 sends them as they are - half the bytes per step - and the device
widens them while it finishes the batch (csrc/batch.hip ``vbw_concap_finish_batch``, csrc/wire16.hip ``vbw_widen_f16``;
include/vilbert_hip_wire.h). Widening is exact, so the batch holds the bits of the default pipeline fed the widened arrays.
``feature_dtype=torch.bfloat16`` writes the feature block as bf16 - what the bf16 stream rounds it to before its first GEMM
anyway (``BertImageEmbeddings`` takes it as it is) - so the fp32 block and the cast launch are never made. The row clearing of
the dynamic masking is fused into that pass (``zero_row``): there is no 16-bit row-clearing launch and the float16 buffer is
never written.
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from .staging import StagedPipeline, out_kind

# order of the raw tuple produced by the dataset workers (concept_cap_dataset.py:243-245)
RAW_FIELDS = ("input_ids", "input_mask", "segment_ids", "lm_label_ids", "is_next", "image_feat", "image_loc",
              "image_target", "image_label", "image_mask", "masked_label")
# the same tuple from a source that selects nothing (unmasked_preprocess): the [regions, regions] IoU matrix of the boxes
# stands where masked_label stood, lm_label_ids / image_label are all -1 and are replaced by mask_batch
RAW_UNMASKED_FIELDS = tuple("overlaps" if n == "masked_label" else n for n in RAW_FIELDS)
_DTYPES = dict(input_ids=torch.int64, input_mask=torch.int64, segment_ids=torch.int64, lm_label_ids=torch.int64,
               is_next=torch.int64, image_feat=torch.float32, image_loc=torch.float32, image_target=torch.float32,
               image_label=torch.int64, image_mask=torch.int64, masked_label=torch.int64, overlaps=torch.float32)
WIRE_FIELDS = ("image_feat", "image_target")      # what travels as float16 with wire_dtype=torch.float16
_MASK64 = 0xFFFFFFFFFFFFFFFF
BATCH_SEED_STRIDE = 0xD1B54A32D192ED03


def batch_seed(seed, i):
    """Seed of batch i of a run seeded with `seed`: the splitmix64 finaliser (all 64 bits) of
    ``seed + (i + 1) * 0xD1B54A32D192ED03`` (mod 2^64). A pure function of (seed, i), so a restarted run reproduces its masks.
    The kernel hashes ``seed + index * 0x9E3779B97F4A7C15``: two seeds a small multiple of that stride apart would draw the
    same mask shifted by a few sites (ops._chunk_seed records that bug), which is why the per-batch term goes through the full
    mixer instead of being added to the seed (tests/test_mask_batch.py checks batches 0 .. 63 pairwise)."""
    z = (int(seed) + (int(i) + 1) * BATCH_SEED_STRIDE) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


class Masking(object):
    """Settings and batch counter of the device-side masking. The g-th batch masked through this object - counted from
    `first_batch`, over every iteration of every DeviceBatchPipeline that holds it - is masked with ``batch_seed(seed, g)``:
    a pure function of (seed, global batch index). The count runs on across iterations, so a second pass over the same
    source draws new masks (``next_batch`` is where it stands); a run that restarts at global batch k passes first_batch=k
    and repeats the masks of the original run from there."""

    def __init__(self, seed, vocab_size, mask_token_id, p_select=0.15, first_batch=0):
        if not 0.0 <= float(p_select) <= 1.0:
            raise ValueError("p_select must lie in [0, 1], got %r" % (p_select,))
        if int(vocab_size) <= 0 or not 0 <= int(mask_token_id) < int(vocab_size):
            raise ValueError("mask_token_id %r is not an id of a vocabulary of %r" % (mask_token_id, vocab_size))
        self.seed, self.vocab_size, self.mask_token_id = int(seed) & _MASK64, int(vocab_size), int(mask_token_id)
        self.p_select, self.first_batch = float(p_select), int(first_batch)
        self.next_batch = self.first_batch

    def batch_seed(self, i):
        """Seed of the i-th batch after `first_batch` (no state is touched)."""
        return batch_seed(self.seed, self.first_batch + i)

    def next_seed(self):
        """Seed of global batch `next_batch`; advances the count."""
        g = self.next_batch
        self.next_batch = g + 1
        return batch_seed(self.seed, g)


def unmasked_preprocess(cls):
    """A subclass of `cls` (a class shaped like the reference's BertPreprocessBatch) whose workers select nothing: its
    samples reach the pipeline unmasked, in RAW_UNMASKED_FIELDS layout. Only the signatures of the two overridden methods
    are relied on; negative captions and tokenisation stay with `cls`."""

    class Unmasked(cls):
        def random_word(self, tokens, tokenizer, is_next):
            return tokens, [-1] * len(tokens)

        def random_region(self, image_feat, image_loc, num_boxes, is_next, overlaps):
            regions = image_feat.shape[0]
            given = np.asarray(overlaps, dtype=np.float32)
            padded = np.zeros((regions, regions), dtype=np.float32)
            r, c = min(regions, given.shape[0]), min(regions, given.shape[1])
            padded[:r, :c] = given[:r, :c]
            return image_feat, image_loc, [-1] * int(num_boxes), padded

    Unmasked.__name__ = "Unmasked" + cls.__name__
    Unmasked.__qualname__ = Unmasked.__name__
    return Unmasked


def mask_batch(raw, seed, vocab_size, mask_token_id, p_select=0.15, inplace=True):
    """raw: dict of DEVICE tensors named as RAW_UNMASKED_FIELDS (unmasked worker output). Draws the MLM and region masks
    (include/vilbert_hip_inputs.h states the rule) and returns the dict `finish_batch` takes. Two native launches on the
    current stream, no torch arithmetic. inplace=True rewrites the buffers of `raw` (input_ids, lm_label_ids, image_label,
    the selected rows of image_feat); inplace=False leaves every tensor of `raw` as it is. image_target is passed through
    untouched in both (the reference copies it before it masks).
    A float16 image_feat is never rewritten, under both `inplace` settings: only the masking launch runs and its row flags
    are returned as ``zero_row`` [batch, regions] uint8 - `finish_batch` writes those rows as zeros while it widens."""
    feat = raw["image_feat"]
    if feat.dim() != 3:
        raise RuntimeError("image_feat must be [batch, regions, feat_dim]")
    B, R, F = feat.shape
    ids = raw["input_ids"]
    if ids.dim() != 2 or ids.shape[0] != B:
        raise RuntimeError("input_ids must be [batch, tokens]")
    T = ids.shape[1]
    dev = feat.device

    def i64(name, shape):
        t = raw[name]
        if tuple(t.shape) != shape:
            raise RuntimeError("%s: expected shape %s, got %s" % (name, shape, tuple(t.shape)))
        return N.dev_i64(t, name)

    half = feat.dtype == torch.float16
    ov = raw["overlaps"]
    if tuple(ov.shape) != (B, R, R) or not ov.is_contiguous() or not feat.is_contiguous():
        raise RuntimeError("overlaps / image_feat: expected contiguous tensors of shape %s / %s, got %s / %s"
                           % ((B, R, R), (B, R, F), tuple(ov.shape), tuple(feat.shape)))

    def out_i64(name, shape):
        t = raw.get(name) if inplace else None
        if t is None or tuple(t.shape) != shape or t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
            t = torch.empty(shape, dtype=torch.int64, device=dev)
        return t

    out_ids, lm, ilab = out_i64("input_ids", (B, T)), out_i64("lm_label_ids", (B, T)), out_i64("image_label", (B, R))
    masked = torch.empty(B, R, dtype=torch.int64, device=dev)
    zero_row = torch.empty(B, R, dtype=torch.uint8, device=dev)
    a = N.MaskArgs()
    a.batch, a.tokens, a.regions = B, T, R
    a.vocab_size, a.mask_token_id, a.p_select, a.seed = int(vocab_size), int(mask_token_id), float(p_select), int(seed) & _MASK64
    a.input_ids, a.input_mask, a.image_mask = i64("input_ids", (B, T)), i64("input_mask", (B, T)), i64("image_mask", (B, R))
    a.overlaps = N.dev_f32(ov, "overlaps")
    a.out_input_ids, a.lm_label_ids, a.image_label = out_ids.data_ptr(), lm.data_ptr(), ilab.data_ptr()
    a.masked_label, a.zero_row = masked.data_ptr(), zero_row.data_ptr()
    N.check(N.lib().vbi_concap_mask_batch(N.stream_ptr(), ctypes.byref(a)), "vbi_concap_mask_batch")
    out = {n: raw[n] for n in RAW_FIELDS if n != "masked_label"}
    if half:
        out_feat = feat
        out["zero_row"] = zero_row
    else:
        out_feat = feat if inplace else torch.empty_like(feat)
        N.check(N.lib().vbi_zero_rows(N.stream_ptr(), B * R, F, N.dev_f32(feat, "image_feat"), F, zero_row.data_ptr(),
                                      None if inplace else out_feat.data_ptr(), F), "vbi_zero_rows")
    out.update(input_ids=out_ids, lm_label_ids=lm, image_label=ilab, image_feat=out_feat, masked_label=masked)
    return out


def widen_f16(x):
    """Contiguous float16 DEVICE tensor -> the fp32 tensor of the same values (exact; one native launch, no torch arithmetic)."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise RuntimeError("widen_f16: expected a tensor on a HIP device - the MI355X-native path has no CPU fallback")
    if x.dtype != torch.float16 or not x.is_contiguous():
        raise RuntimeError("widen_f16: expected a contiguous float16 tensor, got %s" % x.dtype)
    y = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    N.check(N.lib().vbw_widen_f16(N.stream_ptr(), x.numel(), x.data_ptr(), y.data_ptr()), "vbw_widen_f16")
    return y


def finish_batch(raw, objective=0, out_dtype=torch.float32):
    """raw: dict of DEVICE tensors named as RAW_FIELDS (worker output, unchanged). Returns the 10-tuple the
    training loop feeds to the model. One native launch pair on the current stream; no torch arithmetic.
    A float16 image_feat is widened by the finishing pass itself (include/vilbert_hip_wire.h): the tuple holds the bits the
    fp32 path gives on the widened features, or with out_dtype=torch.bfloat16 (float16 features only) those bits rounded to
    bf16. With float16 features an optional raw["zero_row"] [batch, regions] uint8 (``mask_batch``) names the rows that become zeros. A float16
    image_target is widened to fp32 (one more launch)."""
    feat = raw["image_feat"]
    if feat.dim() != 3:
        raise RuntimeError("image_feat must be [batch, regions, feat_dim]")
    half = feat.dtype == torch.float16
    kind = out_kind(out_dtype, half, "finish_batch")
    B, R, F = feat.shape
    T = raw["lm_label_ids"].shape[1]
    dev = feat.device
    target = raw["image_target"]
    if isinstance(target, torch.Tensor) and target.dtype == torch.float16:
        target = widen_f16(target)
    out_feat = torch.empty(B, R + 1, F, dtype=out_dtype, device=dev)
    out_loc = torch.empty(B, R + 1, 5, dtype=torch.float32, device=dev)
    out_mask = torch.empty(B, R + 1, dtype=torch.int64, device=dev)
    out_ilab = torch.empty(B, R, dtype=torch.int64, device=dev)
    out_lm = torch.empty(B, T, dtype=torch.int64, device=dev)
    a = N.WireConcapBatch() if half else N.ConcapBatch()
    a.batch, a.regions, a.tokens, a.feat_dim, a.objective = B, R, T, F, int(objective)

    def f32(name, shape):
        t = raw[name]
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError("%s: expected a contiguous tensor of shape %s, got %s" % (name, shape, tuple(t.shape)))
        return N.dev_f32(t, name)

    def i64(name, shape):
        t = raw[name]
        if tuple(t.shape) != shape:
            raise RuntimeError("%s: expected shape %s, got %s" % (name, shape, tuple(t.shape)))
        return N.dev_i64(t, name)

    if half:
        if not feat.is_cuda or tuple(feat.shape) != (B, R, F) or not feat.is_contiguous():
            raise RuntimeError("image_feat: expected a contiguous float16 tensor on a HIP device")
        a.image_feat, a.out_kind = feat.data_ptr(), kind
        flags = raw.get("zero_row")
        if flags is not None:
            if not flags.is_cuda or flags.dtype != torch.uint8 or tuple(flags.shape) != (B, R) or not flags.is_contiguous():
                raise RuntimeError("zero_row: expected a contiguous uint8 tensor of shape %s on a HIP device" % ((B, R),))
            a.zero_row = flags.data_ptr()
    else:
        a.image_feat = f32("image_feat", (B, R, F))
    a.image_loc = f32("image_loc", (B, R, 5))
    a.image_mask, a.masked_label = i64("image_mask", (B, R)), i64("masked_label", (B, R))
    a.is_next, a.image_label = i64("is_next", (B,)), i64("image_label", (B, R))
    a.lm_label_ids = i64("lm_label_ids", (B, T))
    a.out_image_feat, a.out_image_loc = out_feat.data_ptr(), out_loc.data_ptr()
    a.out_image_mask, a.out_image_label, a.out_lm_label_ids = out_mask.data_ptr(), out_ilab.data_ptr(), out_lm.data_ptr()
    if half:
        N.check(N.lib().vbw_concap_finish_batch(N.stream_ptr(), ctypes.byref(a)), "vbw_concap_finish_batch")
    else:
        N.check(N.lib().vb_concap_finish_batch(N.stream_ptr(), ctypes.byref(a)), "vb_concap_finish_batch")
    return (raw["input_ids"], raw["input_mask"], raw["segment_ids"], out_lm, raw["is_next"], out_feat, out_loc,
            target, out_ilab, out_mask)


class DeviceBatchPipeline(StagedPipeline):
    """Iterate over ``source`` (an iterable of RAW worker batches: tuples of numpy arrays in RAW_FIELDS order,
    optionally followed by extra items such as image ids - what ``self.ds.get_data()`` yields inside the
    reference loader) and yield finished device batches (+ the extra items).

    Batch i+1 is staged on a dedicated stream right after the caller has enqueued step i, so the transfer runs
    under step i (``StagedPipeline``: the double buffering and the two staging modes, "direct" and "pinned").
    The id / mask / target tensors of a yielded batch alias the slot's device buffers: they stay valid
    until the caller asks for batch i + depth - 1 (do not keep them across iterations).

    masking=None: the source masks (the reference's workers), as above. masking=Masking(...): the source yields UNMASKED
    batches in RAW_UNMASKED_FIELDS order (``unmasked_preprocess`` makes such a worker class) and every batch is masked on the
    compute stream by ``mask_batch`` with ``masking.next_seed()`` before it is finished: the Masking object counts the batches
    across iterations (and across pipelines that share it), so each pass over a source draws new masks.

    wire_dtype=None: image_feat and image_target cross the bus as fp32 (a float16 array is widened on the host first).
    wire_dtype=torch.float16: the source supplies float16 arrays for both (anything else raises ValueError - the pipeline
    never narrows), the slot buffers are float16 and the device widens them; the yielded batch holds the bits of the default
    pipeline fed the widened arrays. feature_dtype=torch.bfloat16 (with the float16 wire only) yields image_feat rounded to
    bf16, for the bf16 stream."""

    dtypes, wire_fields, blank_fields = _DTYPES, WIRE_FIELDS, ()

    def __init__(self, source, device, objective=0, depth=2, staging=None, masking=None, wire_dtype=None,
                 feature_dtype=torch.float32):
        StagedPipeline.__init__(self, source, device, depth, staging, wire_dtype, feature_dtype)
        self.objective, self.masking = int(objective), masking
        self.fields = RAW_FIELDS if masking is None else RAW_UNMASKED_FIELDS
        if masking is not None:
            # all -1 from an unmasked source and never read: mask_batch writes every element of the device buffers
            self.blank_fields = ("lm_label_ids", "image_label")

    def arrays(self, batch):
        return dict(zip(self.fields, batch)), tuple(batch[len(self.fields):])

    def finish(self, slot):
        raw, m = slot.views, self.masking
        if m is not None:
            raw = mask_batch(raw, m.next_seed(), m.vocab_size, m.mask_token_id, m.p_select, inplace=True)
        return finish_batch(raw, self.objective, self.feature_dtype) + slot.extra
