"""The one place that knows when a tensor derived from parameters (fp8 / MX codes, bf16 shadows) is stale.

A `DerivedWeights` maps the (stacked) weight segments of a linear to a payload its client built from them. The payload is
served as long as nothing rewrote a segment: torch's version counters are compared per call, and `_native.WEIGHTS_EPOCH`
covers the writers those counters do not see (the native optimizer's raw pointers, optimizers that write through `.data`).
A stale payload is refreshed IN PLACE, so captured graphs keep its addresses. An entry holds an alias of every segment, so
an address cannot be recycled by another tensor while it is cached, and weak references to the tensors the caller passed
(the nn.Parameter objects): entries whose tensors are all gone are dropped at the next miss.

It knows nothing about number formats. The client gives `build(weights, biases, hint) -> payload` and
`refresh(payload, weights, biases)` (the parts that launch kernels), and one of two key rules:
  fits=None: key (id(first weight), number of segments); a hit needs every segment to be the very tensor the entry was
             built from (an id can be recycled);
  fits=f:    key = the segments' addresses; a hit needs f(payload, weights, hint) - the same address may be another view
             of a buffer.
"""
import weakref

import torch

from . import _native as N

_EPOCH = N.WEIGHTS_EPOCH


def _weight_versions(weights, biases):
    return tuple(w._version for w in weights)


def _weight_and_bias_versions(weights, biases):
    return tuple(w._version for w in weights) + tuple(-1 if b is None else b._version for b in (biases or ()))


class Entry(object):
    __slots__ = ("payload", "vers", "epoch", "keep", "wrefs", "device")

    def alive(self):
        return all(r() is not None for r in self.wrefs)

    def dead(self):
        return all(r() is None for r in self.wrefs)


class DerivedWeights(object):
    def __init__(self, build, refresh, fits=None, bias_versions=False, on_epoch=None):
        """bias_versions: the payload holds a copy of the biases too, their version counters count.
        on_epoch(device): called before the refresh of an entry whose epoch is behind - a client that can refresh all its
        entries of a device at once does so there and `stamp`s them; an entry it did not stamp is refreshed on its own."""
        self._entries = {}
        self._build, self._refresh, self._fits = build, refresh, fits
        self._versions = _weight_and_bias_versions if bias_versions else _weight_versions
        self._on_epoch = on_epoch

    def get(self, weights, biases=None, hint=None):
        """The payload of these segments, built or refreshed if it has to be. `hint` goes to `fits` and `build` unread."""
        if self._fits is None:
            key = (id(weights[0]), len(weights))
            e = self._entries.get(key)
            if e is not None and any(r() is not w for r, w in zip(e.wrefs, weights)):
                e = None                                   # a recycled id
        else:
            key = tuple(w.data_ptr() for w in weights)
            e = self._entries.get(key)
            if e is not None and not self._fits(e.payload, weights, hint):
                e = None                                   # same address, different view of a buffer
        epoch = _EPOCH[0]
        if e is not None:
            if e.epoch != epoch and self._on_epoch is not None:
                with torch.no_grad():
                    self._on_epoch(e.device)
            if e.epoch == epoch and e.vers == self._versions(weights, biases):
                return e.payload
        with torch.no_grad():
            if e is not None:
                self._refresh(e.payload, weights, biases)
            else:
                self.drop([k for k, old in self._entries.items() if old.dead()])
                e = Entry()
                e.payload, e.device = self._build(weights, biases, hint), weights[0].device
        e.keep = [w.detach() for w in weights]
        e.wrefs = [weakref.ref(w) for w in weights]
        e.vers, e.epoch = self._versions(weights, biases), epoch
        self._entries[key] = e
        return e.payload

    def entries(self, device):
        """[(key, entry)] of the entries built from weights on `device`."""
        return [(k, e) for k, e in self._entries.items() if e.device.index == device.index]

    def stamp(self, entries):
        """The client refreshed the payloads of these (live, bias-free) entries itself: they are current as of now."""
        epoch = _EPOCH[0]
        for e in entries:
            e.vers, e.epoch = self._versions([r() for r in e.wrefs], None), epoch
        return epoch

    def drop(self, keys):
        for k in keys:
            del self._entries[k]

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)
