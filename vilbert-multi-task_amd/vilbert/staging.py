"""The double-buffered staging loop of the device-side input pipelines (``vilbert.input_pipeline.DeviceBatchPipeline``,
``vilbert.task_pipeline.TaskBatchPipeline``): the numpy arrays of batch i + 1 are copied to the device on a dedicated HIP stream
right after the caller has enqueued step i, so the transfer runs under step i, and a native pass finishes the batch on the
compute stream. One protocol, stated here once; a pipeline adds which arrays it stages and how it finishes them.
"""
import os

import numpy as np
import torch

from . import _native as N


def out_kind(out_dtype, half, what):
    """The out_kind word of include/vilbert_hip_wire.h for a feature block of `out_dtype`; `half`: the features are float16."""
    if out_dtype not in N.WIRE_OUT_KINDS:
        raise ValueError("%s: out_dtype must be torch.float32 or torch.bfloat16, got %r" % (what, out_dtype))
    if out_dtype != torch.float32 and not half:
        raise ValueError("%s: out_dtype=%s needs float16 features (fp32 features give an fp32 block)" % (what, out_dtype))
    return N.WIRE_OUT_KINDS[out_dtype]


class _Slot(object):
    """The device buffers of one batch in flight (``dev``), their pinned host twins (``host``; "pinned" staging only) and the
    views of them the current batch uses (``views``). ``copied``: the H2D copy of the current contents has finished (the host
    may refill the pinned buffers; compute waits on it). ``released``: the step that read the device buffers has run (the
    copy stream waits on it before overwriting them)."""

    def __init__(self):
        self.host, self.dev, self.views, self.copied, self.released, self.extra = {}, {}, {}, None, None, ()

    def ensure(self, name, shape, dtype, device, pinned):
        """Leading views [shape[0]] of the pinned (None unless `pinned`) and the device buffer of `name`. The buffers are sized
        by CAPACITY: reallocated only when the batch does not fit (more rows than ever before, other trailing dimensions or
        another dtype), so a batch of the shape of the last one uses them whole."""
        d = self.dev.get(name)
        if d is None or d.dtype != dtype or tuple(d.shape[1:]) != tuple(shape[1:]) or d.shape[0] < shape[0]:
            cap = (max(int(shape[0]), 1),) + tuple(shape[1:])
            self.dev[name] = d = torch.empty(cap, dtype=dtype, device=device)
            self.host.pop(name, None)
        h = self.host.get(name)
        if pinned and h is None:
            self.host[name] = h = torch.empty(d.shape, dtype=dtype).pin_memory()
        return (h[:shape[0]] if pinned else None), d[:shape[0]]


class StagedPipeline(object):
    """Iterates over ``source`` and yields ``finish(slot)`` per batch. A subclass sets
        fields        the names of the arrays of a batch that get a device buffer, in staging order
        dtypes        name -> torch dtype of the device buffer (a name that is missing keeps its array's own dtype)
        wire_fields   the names that travel as float16 with wire_dtype=torch.float16 (anything else from the source raises
                      ValueError: a pipeline never narrows)
        blank_fields  names whose device buffer is only made - the finishing pass writes every element of it
    and implements ``arrays(batch)`` -> (mapping name -> numpy array, the extra items kept as ``slot.extra``) and
    ``finish(slot)`` -> the tuple to yield, from ``slot.views`` on the current stream.

    Two staging modes (``staging``, default: environment variable VB_PIPE_STAGING, else "direct"): "direct" hands the pageable
    numpy memory to the runtime's own copy path (it stages through its internal pinned chunks and does any dtype conversion;
    blocks the host for the duration of the transfer but never makes the CPU write through an uncached host mapping) and
    "pinned" (numpy -> pinned buffer -> asynchronous DMA; on this platform the CPU's writes into the pinned mapping are the
    slow part: 131 vs 137-154 ms per pre-training step at batch 256). Staging from a background thread was measured and is
    slower still: the step's ~1500 kernel launches are Python-side work and lose more to GIL hand-offs than the overlap wins
    (161 vs 137 ms). The tensors of ``slot.views`` alias the slot's device buffers: what a pipeline yields of them stays valid
    until the caller asks for batch i + depth - 1."""

    fields, dtypes, wire_fields, blank_fields = (), {}, (), ()

    def __init__(self, source, device, depth, staging, wire_dtype, feature_dtype):
        self.source, self.device = source, torch.device(device)
        if wire_dtype not in (None, torch.float16):
            raise ValueError("wire_dtype must be None or torch.float16, got %r" % (wire_dtype,))
        out_kind(feature_dtype, wire_dtype is not None, type(self).__name__)
        self.wire_dtype, self.feature_dtype = wire_dtype, feature_dtype
        self._copy_stream = None
        self.slots = [_Slot() for _ in range(max(2, depth))]
        self.staging = staging or os.environ.get("VB_PIPE_STAGING", "direct")

    @property
    def copy_stream(self):
        if self._copy_stream is None:                       # made on first use: the constructor touches no device
            self._copy_stream = torch.cuda.Stream(device=self.device)
        return self._copy_stream

    def _stage(self, slot, batch):
        arrays, extra = self.arrays(batch)
        if self.wire_dtype is not None:
            for name in self.wire_fields:
                if np.asarray(arrays[name]).dtype != np.float16:
                    raise ValueError("%s: wire_dtype=torch.float16 takes a float16 array from the source, got %s (the pipeline "
                                     "never narrows)" % (name, np.asarray(arrays[name]).dtype))
        if slot.copied is not None:
            slot.copied.synchronize()                       # pinned buffers free again (long done)
        if slot.released is not None:
            self.copy_stream.wait_event(slot.released)      # device buffers free once that step has run
        slot.extra, slot.views = extra, {}
        with torch.cuda.stream(self.copy_stream):
            for name in self.fields:
                if name in self.blank_fields:
                    slot.views[name] = slot.ensure(name, np.shape(arrays[name]), self.dtypes[name], self.device, False)[1]
                    continue
                src = torch.from_numpy(np.ascontiguousarray(arrays[name]))
                dtype = self.wire_dtype if self.wire_dtype is not None and name in self.wire_fields \
                    else self.dtypes.get(name, src.dtype)
                h, d = slot.ensure(name, src.shape, dtype, self.device, self.staging != "direct")
                if h is None:
                    d.copy_(src, non_blocking=False)        # "direct": dtype conversion (e.g. int32 ids), if any, is the runtime's
                else:
                    h.copy_(src)                            # dtype conversion happens here
                    d.copy_(h, non_blocking=True)
                slot.views[name] = d
            slot.copied = torch.cuda.Event()
            slot.copied.record(self.copy_stream)

    def __iter__(self):
        it = iter(self.source)
        batch = next(it, None)
        if batch is None:
            return
        idx = 0
        self._stage(self.slots[0], batch)
        while True:
            slot = self.slots[idx]
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(slot.copied)
            for t in slot.dev.values():
                t.record_stream(cur)      # allocated on the copy stream, read by kernels of the compute stream
            yield self.finish(slot)
            slot.released = torch.cuda.Event()
            slot.released.record(torch.cuda.current_stream(self.device))   # after the caller's step
            batch = next(it, None)
            if batch is None:
                return
            idx = (idx + 1) % len(self.slots)
            self._stage(self.slots[idx], batch)
