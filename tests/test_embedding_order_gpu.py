"""Ordered text-embedding backward (vb_text_embed_bwd under the deterministic setting): the four gradient tables are a
keyed reduction whose order include/vilbert_hip.h documents. Each case compares the kernels BITWISE with a numpy
float32 restatement of that order (sequential sums only: np.cumsum, never np.sum), checks that repeated calls agree, that
the atomic path (setting off) agrees to fp32 tolerance, and that a workspace too small for the call falls back to the
atomics and is counted."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RUN = 64        # rows per run (EMB_RUN, csrc/embed_bwd.hip)


@pytest.fixture
def det():
    from vilbert import _native
    wanted = _native._DET["wanted"]
    _native.set_deterministic(True)
    yield _native
    _native.set_deterministic(wanted)


def _ordered_sum(x):
    """One key: rows in ascending r, runs of RUN rows summed left to right, run sums added left to right (float32)."""
    runs = np.stack([np.cumsum(x[j:j + RUN], axis=0, dtype=np.float32)[-1] for j in range(0, len(x), RUN)])
    return np.cumsum(runs, axis=0, dtype=np.float32)[-1]


def _reduce_into(table, keys, x):
    """table[k] = table[k] + ordered sum of the rows x[r] with keys[r] == k (keys < 0: skipped)."""
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    first = np.searchsorted(ks, 0)
    bounds = np.flatnonzero(np.diff(ks[first:])) + first + 1
    starts = np.concatenate([[first], bounds]) if first < len(ks) else np.array([], dtype=np.int64)
    ends = np.concatenate([bounds, [len(ks)]]) if first < len(ks) else np.array([], dtype=np.int64)
    for s, e in zip(starts, ends):
        k = ks[s]
        table[k] = table[k] + _ordered_sum(x[order[s:e]])


def _restated(dx, ids, seg, task_ids, tables):
    """numpy float32 restatement of the documented order; `tables` = incoming [word, pos, type, task] (task may be None)."""
    word, pos, typ, task = [None if t is None else t.copy() for t in tables]
    B, T = ids.shape
    n_out = T + (1 if task_ids is not None else 0)
    H = dx.shape[-1]
    x = dx.reshape(B * n_out, H)
    b = np.repeat(np.arange(B), n_out)
    t_out = np.tile(np.arange(n_out), B)
    is_task = (t_out == 1) if task_ids is not None else np.zeros_like(t_out, dtype=bool)
    t = np.where((task_ids is not None) & (t_out >= 2), t_out - 1, t_out)
    t = np.where(is_task, 0, t)
    idv, sv = ids[b, t], seg[b, t]
    wkey = np.where(~is_task & (idv > 0) & (idv < word.shape[0]), idv, -1)
    pkey = np.where(~is_task, t, -1)
    tkey = np.where(~is_task & (sv >= 0) & (sv < typ.shape[0]), sv, -1)
    _reduce_into(word, wkey, x)
    _reduce_into(pos, pkey, x)
    _reduce_into(typ, tkey, x)
    if task_ids is not None:
        tv = task_ids.reshape(-1)[b]
        _reduce_into(task, np.where(is_task & (tv >= 0) & (tv < task.shape[0]), tv, -1), x)
    return word, pos, typ, task


def _ids(B, T, V, g):
    """Token ids as the pre-training loader makes them: [CLS], random words, [SEP], ~12 % [MASK], zero padding."""
    ids = torch.randint(104, V, (B, T), generator=g)
    ids[:, 0] = 101
    lens = torch.randint(T // 2, T + 1, (B,), generator=g)
    for i in range(B):
        ids[i, lens[i] - 1] = 102
        ids[i, lens[i]:] = 0
    mask = (torch.rand(B, T, generator=g) < 0.12) & (ids > 102)
    return torch.where(mask, torch.full_like(ids, 103), ids)


def _case(B, T, H, V, n_types, n_tasks=0, P=None, seed=0, bad=False, hot=False, init=False):
    g = torch.Generator().manual_seed(seed)
    ids = _ids(B, T, V, g)
    seg = torch.randint(0, max(n_types, 2), (B, T), generator=g)
    task_ids = torch.randint(0, n_tasks, (B, 1), generator=g) if n_tasks else None
    n_out = T + (1 if n_tasks else 0)
    dx = torch.randn(B, n_out, H, generator=g)
    if hot:
        # one id at every position; values of mixed magnitude: any other summation order shows in the bits
        ids[:] = 7
        big = torch.rand(B, n_out, H, generator=g) < 0.5
        dx = torch.where(big, dx * 1e6, dx * 1e-3)
    if bad:
        ids[0, 1], ids[1, 2], ids[2, 3], ids[3, 0] = V + 5, -3, V, 0
        seg[0, 2], seg[1, 3], seg[2, 4] = -1, n_types, n_types + 7
        if task_ids is not None:
            task_ids[0, 0], task_ids[1, 0] = -1, n_tasks
    P = P or T + 4
    shapes = [(V, H), (P, H), (n_types, H), (n_tasks, H) if n_tasks else None]
    tables = [(torch.randn(*s, generator=g) if init else torch.zeros(*s)) if s else None for s in shapes]
    return dx, ids, seg, task_ids, shapes, tables


def _run(dx, ids, seg, task_ids, shapes, tables):
    from vilbert import ops
    out = [t.to(DEV) if t is not None else None for t in tables]
    got = ops.text_embed_bwd(dx.to(DEV), ids.to(DEV), seg.to(DEV), task_ids.to(DEV) if task_ids is not None else None,
                             shapes[0], shapes[1], shapes[2], shapes[3], out=out)
    torch.cuda.synchronize()
    return [g.cpu() if g is not None else None for g in got]


CASES = {
    "timed_b256_t36_h768": dict(B=256, T=36, H=768, V=30522, n_types=2),
    "hidden_1024": dict(B=64, T=36, H=1024, V=30522, n_types=2),
    "rows_64k": dict(B=512, T=128, H=768, V=30522, n_types=2, P=512),
    "task_tokens": dict(B=48, T=20, H=768, V=30522, n_types=2, n_tasks=20),
    "one_type_row_roberta": dict(B=32, T=36, H=768, V=50265, n_types=1),
    "three_types": dict(B=32, T=36, H=768, V=30522, n_types=3),
    "out_of_range_and_padding": dict(B=16, T=12, H=256, V=1000, n_types=2, n_tasks=4, bad=True),
    "accumulating_tables": dict(B=64, T=36, H=768, V=30522, n_types=2, n_tasks=8, init=True),
    "hot_id_mixed_magnitude": dict(B=256, T=36, H=768, V=30522, n_types=2, hot=True),
    "hot_id_64k_rows": dict(B=512, T=128, H=256, V=30522, n_types=3, P=512, hot=True, init=True),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_match_the_documented_order_bitwise(det, name):
    dx, ids, seg, task_ids, shapes, tables = _case(**CASES[name])
    before = det.deterministic_fallbacks()
    got = _run(dx, ids, seg, task_ids, shapes, tables)
    assert det.deterministic_fallbacks() == before, "the ordered path fell back to atomics"
    want = _restated(dx.numpy(), ids.numpy(), seg.numpy(), task_ids.numpy() if task_ids is not None else None,
                     [t.numpy() if t is not None else None for t in tables])
    for label, g, w in zip(("word", "position", "type", "task"), got, want):
        if w is None:
            assert g is None
            continue
        diff = np.flatnonzero((g.numpy() != w).any(axis=1))
        assert diff.size == 0, "%s table: rows %s differ from the documented order" % (label, diff[:10].tolist())


def test_repeated_calls_are_identical_and_the_atomic_path_agrees(det):
    dx, ids, seg, task_ids, shapes, tables = _case(B=256, T=36, H=768, V=30522, n_types=3, n_tasks=6, seed=3)
    runs = [_run(dx, ids, seg, task_ids, shapes, tables) for _ in range(3)]
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)
    det.set_deterministic(False)
    try:
        atomic = _run(dx, ids, seg, task_ids, shapes, tables)
    finally:
        det.set_deterministic(True)
    for a, b in zip(runs[0], atomic):
        assert (a - b).abs().max().item() <= 1e-4 * max(1.0, b.abs().max().item())


def test_workspace_too_small_falls_back_to_atomics_and_is_counted():
    from vilbert import _native
    prev = _native._DET["wanted"]
    _native.set_deterministic(False)
    ws = torch.empty(8 * 1024, dtype=torch.float32, device=DEV)
    assert _native.lib().vb_set_deterministic(1, ws.data_ptr(), ws.numel() * 4) == 0
    try:
        assert _native.deterministic_fallbacks() == 0
        dx, ids, seg, task_ids, shapes, tables = _case(B=64, T=36, H=768, V=30522, n_types=2, seed=4)
        got = _run(dx, ids, seg, task_ids, shapes, tables)
        assert _native.deterministic_fallbacks() >= 1
        want = _restated(dx.numpy(), ids.numpy(), seg.numpy(), None, [t.numpy() if t is not None else None for t in tables])
        for g, w in zip(got[:3], want[:3]):
            assert np.abs(g.numpy() - w).max() <= 1e-4 * max(1.0, np.abs(w).max())
    finally:
        _native.lib().vb_set_deterministic(0, None, 0)
        _native.set_deterministic(prev)
