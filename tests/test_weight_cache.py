"""vilbert/weight_cache.py on CPU tensors: when a tensor derived from parameters (the fp8 / MX codes, the bf16 shadows)
is served, refreshed in place, rebuilt or dropped - under both key rules (segment addresses + a shape test: the fp8 and MX
caches; (id of the first weight, segment count) + identity: the bf16 shadows). build / refresh copy the weight and count."""
import gc

import pytest
import torch

from vilbert import _native
from vilbert.weight_cache import DerivedWeights


def _stacked(weights):
    return torch.cat([w.detach() for w in weights])


def _fits(payload, weights, hint):
    return payload.shape == (len(weights) * weights[0].shape[0], weights[0].shape[1])


class _Counting(object):
    def __init__(self, rule):
        self.builds = self.refreshes = 0
        self.cache = DerivedWeights(self.build, self.refresh, fits=_fits if rule == "address" else None)

    def build(self, weights, biases, hint):
        self.builds += 1
        return _stacked(weights).clone()

    def refresh(self, payload, weights, biases):
        self.refreshes += 1
        payload.copy_(_stacked(weights))

    def calls(self):
        return self.builds, self.refreshes


RULES = ["address", "identity"]


def _param(rows=8, cols=4, seed=0):
    return torch.nn.Parameter(torch.randn(rows, cols, generator=torch.Generator().manual_seed(seed)))


@pytest.mark.parametrize("rule", RULES)
def test_hit_makes_no_call(rule):
    c, w = _Counting(rule), _param()
    p = c.cache.get([w])
    assert c.calls() == (1, 0) and torch.equal(p, w.detach())
    for _ in range(3):
        assert c.cache.get([w]) is p
    assert c.calls() == (1, 0)


@pytest.mark.parametrize("rule", RULES)
def test_in_place_update_refreshes_in_place(rule):
    c, w = _Counting(rule), _param()
    p = c.cache.get([w])
    ptr = p.data_ptr()
    with torch.no_grad():
        w.add_(1.0)                                   # bumps torch's version counter
    q = c.cache.get([w])
    assert c.calls() == (1, 1)
    assert q is p and q.data_ptr() == ptr and torch.equal(q, w.detach())
    assert c.cache.get([w]) is p and c.calls() == (1, 1)


@pytest.mark.parametrize("rule", RULES)
def test_write_through_an_alias_needs_the_epoch(rule):
    c, w = _Counting(rule), _param()
    p = c.cache.get([w])
    before = p.clone()
    v0 = w._version
    w.data.add_(1.0)                                  # an optimizer that writes through .data: no version bump
    assert w._version == v0
    assert c.cache.get([w]) is p and c.calls() == (1, 0) and torch.equal(p, before)     # (stale, and nothing can tell)
    _native.weights_changed()
    ptr = p.data_ptr()
    q = c.cache.get([w])
    assert c.calls() == (1, 1) and q is p and q.data_ptr() == ptr and torch.equal(q, w.detach())
    assert c.cache.get([w]) is p and c.calls() == (1, 1)


@pytest.mark.parametrize("rule", RULES)
def test_bias_versions_count_only_where_asked(rule):
    w, b = _param(), torch.nn.Parameter(torch.zeros(8))
    for bias_versions, refreshes in ((True, 1), (False, 0)):
        c = _Counting(rule)
        c.cache = DerivedWeights(c.build, c.refresh, fits=_fits if rule == "address" else None, bias_versions=bias_versions)
        c.cache.get([w], [b])
        with torch.no_grad():
            b.add_(1.0)
        c.cache.get([w], [b])
        assert c.calls() == (1, refreshes)


@pytest.mark.parametrize("rule", RULES)
def test_another_stacking_of_the_same_first_weight_is_its_own_entry(rule):
    c, w, w2 = _Counting(rule), _param(seed=1), _param(seed=2)
    p1 = c.cache.get([w])
    p2 = c.cache.get([w, w2])
    assert c.calls() == (2, 0) and len(c.cache) == 2 and p2 is not p1
    assert torch.equal(p1, w.detach()) and torch.equal(p2, torch.cat([w.detach(), w2.detach()]))
    assert c.cache.get([w]) is p1 and c.cache.get([w, w2]) is p2 and c.calls() == (2, 0)


def test_address_rule_other_view_of_the_same_buffer_is_a_miss():
    c = _Counting("address")
    buf = torch.arange(32, dtype=torch.float32)
    a, b = buf.view(8, 4), buf.view(4, 8)
    assert a.data_ptr() == b.data_ptr()
    pa = c.cache.get([a])
    pb = c.cache.get([b])                             # same key, a payload that does not fit
    assert c.calls() == (2, 0) and pb is not pa and pb.shape == (4, 8) and torch.equal(pb, b)
    assert c.cache.get([b]) is pb and c.calls() == (2, 0)


def test_identity_rule_recycled_id_is_a_miss():
    c, a, b = _Counting("identity"), _param(seed=3), _param(seed=4)
    pa = c.cache.get([a])
    # what CPython does when `a` dies and a new tensor gets its id: the old entry sits under the new tensor's key
    entries = c.cache._entries
    entries[(id(b), 1)] = entries.pop((id(a), 1))
    pb = c.cache.get([b])
    assert c.calls() == (2, 0) and pb is not pa and torch.equal(pb, b.detach())
    assert c.cache.get([b]) is pb and c.calls() == (2, 0)


@pytest.mark.parametrize("rule", RULES)
def test_dead_entries_are_swept_at_the_next_miss_and_clear_empties(rule):
    c = _Counting(rule)
    gone = [_param(seed=s) for s in range(3)]
    stays = _param(seed=9)
    for w in gone:
        c.cache.get([w])
    c.cache.get([stays])
    c.cache.get([gone[0], gone[1]])
    assert len(c.cache) == 5
    del w, gone
    gc.collect()
    assert len(c.cache) == 5 and c.cache.get([stays]) is not None and len(c.cache) == 5       # a hit sweeps nothing
    new = _param(seed=10)
    c.cache.get([new])                                # a miss: the four entries whose tensors are all gone leave
    assert len(c.cache) == 2
    assert c.cache.get([stays]) is not None and c.calls() == (6, 0)
    c.cache.clear()
    assert len(c.cache) == 0
    c.cache.get([stays])
    assert c.calls() == (7, 0)


def test_epoch_hook_refreshes_all_at_once_and_unstamped_entries_fall_back():
    """The bf16 shadows' protocol: on an epoch bump the client refreshes every live entry of the device itself and stamps
    them; an entry it left out (registered after its table was built) is refreshed on its own."""
    c, hooked = _Counting("identity"), []
    w, w2, late = _param(seed=1), _param(seed=2), _param(seed=3)

    def on_epoch(device):
        hooked.append(device)
        mine = [e for _k, e in c.cache.entries(device) if e.alive() and e.payload is not p_late]
        for e in mine:
            e.payload.copy_(_stacked([r() for r in e.wrefs]))
        c.cache.stamp(mine)

    c.cache = DerivedWeights(c.build, c.refresh, on_epoch=on_epoch)
    p, p2, p_late = c.cache.get([w]), c.cache.get([w2]), c.cache.get([late])
    for t in (w, w2, late):
        t.data.mul_(2.0)
    _native.weights_changed()
    assert c.cache.get([w]) is p and torch.equal(p, w.detach())
    assert len(hooked) == 1 and c.calls() == (3, 0)
    assert c.cache.get([w2]) is p2 and torch.equal(p2, w2.detach())        # stamped by the first call's hook
    assert len(hooked) == 1 and c.calls() == (3, 0)
    assert c.cache.get([late]) is p_late and torch.equal(p_late, late.detach())
    assert len(hooked) == 2 and c.calls() == (3, 1)
