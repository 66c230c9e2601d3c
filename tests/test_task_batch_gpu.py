"""The device-side fine-tuning batch builder on the GPU (csrc/task_batch.hip, vilbert.task_pipeline): every output equals the
numpy restatement (tests/task_batch_restatement.py) EXACTLY - the work is copies, zeros, an fp32 sum in row order and single
correctly rounded fp32 operations, so there is no tolerance anywhere in this file - and the inputs recorded from the reference's
own datasets (tests/golden/task_batch.npz) give the recorded outputs through the kernels."""
import ctypes

import numpy as np
import pytest
import torch

import task_batch_restatement as tr
from test_task_batch import GOLDEN, golden_refer_batch, golden_sample, same_bits

pytestmark = pytest.mark.gpu
OUT_NAMES = ("features", "spatials", "image_mask", "target")


def _to_dev(packed):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in packed.items() if v is not None}


def _native_finish(packed, R, ref_box=None, iou_floor=0.0, with_iou=None):
    """vbd_task_finish_batch through the C ABI into buffers pre-filled with NaN (the mask with -7), each between two canary
    margins: what comes back proves that every element is written and nothing around the outputs is."""
    from vilbert import _native as N
    dev = _to_dev(packed)
    B, F, margin = len(packed["offsets"]) - 1, packed["feat"].shape[1], 64
    with_iou = (ref_box is not None) if with_iou is None else with_iou
    shapes = [(B, R, F), (B, R, 5), (B, R), (B, R, 1)]
    flats = [torch.full((2 * margin + int(np.prod(s)),), float("nan") if i != 2 else -7,
                        dtype=torch.float32 if i != 2 else torch.int64, device="cuda") for i, s in enumerate(shapes)]
    a = N.TaskBatchArgs()
    a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.total_rows = B, R, F, iou_floor, packed["feat"].shape[0]
    a.feat, a.boxes, a.offsets, a.image_wh = (dev[n].data_ptr() for n in ("feat", "boxes", "offsets", "image_wh"))
    if "mean_rows" in dev:
        a.mean_rows = dev["mean_rows"].data_ptr()
    a.out_feat, a.out_spatials, a.out_mask = (f[margin:].data_ptr() for f in flats[:3])
    if ref_box is not None:
        rb = torch.from_numpy(np.asarray(ref_box, dtype=np.float32)).cuda()
        a.ref_box = rb.data_ptr()
    if with_iou:
        a.out_iou = flats[3][margin:].data_ptr()
    code = N.lib().vbd_task_finish_batch(N.stream_ptr(), ctypes.byref(a))
    torch.cuda.synchronize()
    outs = []
    for f, s in zip(flats, shapes):
        host = f.cpu().numpy()
        edge = np.concatenate([host[:margin], host[margin + int(np.prod(s)):]])
        assert (edge == -7).all() if host.dtype == np.int64 else np.isnan(edge).all(), "a canary margin was written"
        outs.append(host[margin:margin + int(np.prod(s))].reshape(s))
    return code, outs


def _check(packed, R, ref_box=None, iou_floor=0.0):
    from vilbert import task_pipeline as tp
    want = tr.finish_task_batch(packed, R, ref_box=ref_box, iou_floor=iou_floor)
    code, got = _native_finish(packed, R, ref_box, iou_floor)
    assert code == 0
    for g, w, name in zip(got, want, OUT_NAMES):
        same_bits(g, w, name)
    if ref_box is None:
        assert np.isnan(got[3]).all()                                  # no target asked for: the buffer was not passed
    rb = None if ref_box is None else torch.from_numpy(np.asarray(ref_box, dtype=np.float32)).cuda()
    api = tp.finish_task_batch(_to_dev(packed), R, ref_box=rb, iou_floor=iou_floor)
    assert len(api) == len(want)
    for g, w, name in zip(api, want, OUT_NAMES):
        same_bits(g.cpu().numpy(), w, "api " + name)
    return want


# ---- features, spatials, mask --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 2, 5, 101])
@pytest.mark.parametrize("F", [4, 1028, 2048])
def test_inputs_equal_the_restatement_exactly(F, R):
    """F = 1028 is five 64-lane blocks of 256 columns, the last with one active lane (and is past 256 threads x 4 columns);
    n_b below, at and above what R keeps (n_b + 1 = R - 1, R, R + 1, R + 6) and n_b = 1; R = 101 walks the unrolled row loop
    through full and partial groups of eight rows. Batches of three samples with mean_rows < n_b where n_b > 1 (rows that are
    copied but not summed; with n_b + 1 > R rows that are summed but not copied), and single samples without mean_rows."""
    sizes = [n for n in (1, R - 2, R - 1, R, R + 5) if n > 0]
    sizes = sizes + sizes[:(-len(sizes)) % 3]
    for i in range(0, len(sizes), 3):
        n_rows = sizes[i:i + 3]
        mean = [max(1, n - 1 - (j % 2)) for j, n in enumerate(n_rows)]
        packed = tr.make_packed(n_rows, F, seed=100 * R + F + i, mean_rows=mean, big_image=1)
        want = _check(packed, R)
        assert want[2].sum(1).tolist() == [min(n + 1, R) for n in n_rows]
    for n in (sizes[0], max(sizes)):
        _check(tr.make_packed([n], F, seed=n + R), R)                  # B = 1, mean_rows NULL


def test_image_area_beyond_2_to_24_is_rounded_once():
    packed = tr.make_packed([4, 3], 8, seed=5, big_image=0)
    assert int(packed["image_wh"][0].astype(np.int64).prod()) > 2 ** 24
    want = _check(packed, 6)
    assert (want[1][0, 1:5, 4] > 0).all()


def test_golden_inputs_give_the_reference_outputs():
    from vilbert import task_pipeline as tp
    g = dict(np.load(GOLDEN))
    R = int(g["max_regions"])
    packed = tp.pack_task_samples([golden_sample(g, i) for i in g["vqa_image"]])
    code, got = _native_finish(packed, R)
    assert code == 0
    for a, name in zip(got, ("vqa_features", "vqa_spatials", "vqa_image_mask")):
        same_bits(a, g[name], name)
    labels, scores = torch.from_numpy(g["vqa_labels"]).cuda(), torch.from_numpy(g["vqa_scores"]).cuda()
    same_bits(tp.dense_target(labels, scores, int(g["num_labels"])).cpu().numpy(), g["vqa_target"], "vqa_target")
    for split in ("val", "train"):
        packed, ref_box, floor, want = golden_refer_batch(g, split)
        code, got = _native_finish(packed, R, ref_box, floor)
        assert code == 0
        for a, b, name in zip(got, want, OUT_NAMES):
            same_bits(a, b, "%s %s" % (split, name))


# ---- the region-IoU target -----------------------------------------------------------------------------------------------------
def _boxes_batch(samples, wh):
    """One sample per entry of `samples` (a list of pixel boxes each), 4 feature columns."""
    n_rows = [len(s) for s in samples]
    packed = tr.make_packed(n_rows, 4, seed=3)
    packed["boxes"] = np.concatenate([np.asarray(s, dtype=np.float32).reshape(-1, 4) for s in samples])
    packed["image_wh"] = np.asarray(wh, dtype=np.int32)
    return packed


@pytest.mark.parametrize("floor", [0.0, 0.5])
def test_iou_target_cases(floor):
    ref = [10, 10, 19, 19]
    anchors = [[30, 30, 39, 39],           # disjoint
               [20, 10, 29, 19],           # one pixel apart: iw is exactly 0
               [19, 10, 28, 19],           # touching: one shared column, 10 / 190
               [10, 10, 19, 19],           # identical: 1
               [10, 10, 19, 29],           # the reference box is its upper half: 100 / 200 = 0.5 exactly
               [12.5, 11.25, 22.75, 17.5], [0, 0, 99, 99]]
    packed = _boxes_batch([anchors, [[0, 0, 0, 1], [3, 3, 8, 8]], [[4, 4, 6, 6], [5, 5, 5, 5], [0, 0, 9, 9]]],
                          [(100, 100), (50, 40), (10, 10)])
    # sample 1: anchor [0, 0, 0, 1] against [0, 0, 0, 0] is exactly 0.5; sample 2: a zero-size reference box (one pixel)
    ref_box = np.array([ref, [0, 0, 0, 0], [5, 5, 5, 5]], dtype=np.float32)
    want = _check(packed, 9, ref_box=ref_box, iou_floor=floor)
    t = want[3][..., 0]
    assert t[0, 1] == 0 and t[0, 2] == 0 and t[0, 4] == 1 and t[0, 5] == 0.5 and t[1, 1] == 0.5 and t[2, 2] == 1
    assert (t[0, 8:] == 0).all() and (t[1, 3:] == 0).all()                        # padding rows
    if floor == 0.0:
        assert t[2, 0] == np.float32(1) / np.float32(121)                         # the global row: 0, 0, W, H
        assert t[0, 3] == np.float32(10) / np.float32(190) and 0 < t[0, 6] < 0.5 and 0 < t[2, 1] < 0.5   # untouched
    else:
        assert t[0, 3] == 0 and t[0, 6] == 0 and t[2, 1] == 0 and t[0, 5] == 0.5 and t[1, 1] == 0.5     # exactly 0.5 survives


def test_without_a_reference_box_no_target_is_written():
    from vilbert import task_pipeline as tp
    packed = tr.make_packed([3, 2], 8, seed=9)
    ref_box = np.array([[5, 5, 90, 90], [0, 0, 50, 50]], dtype=np.float32)
    dev = _to_dev(packed)
    with_target = tp.finish_task_batch(dev, 5, ref_box=torch.from_numpy(ref_box).cuda())
    before = with_target[3].clone()
    assert len(tp.finish_task_batch(dev, 5)) == 3
    torch.cuda.synchronize()
    assert torch.equal(with_target[3], before)
    # exactly one of ref_box / out_iou: refused before anything is launched, every buffer keeps its NaNs
    for kwargs in (dict(ref_box=ref_box, with_iou=False), dict(ref_box=None, with_iou=True)):
        code, got = _native_finish(packed, 5, **kwargs)
        assert code == -1 and all(np.isnan(o).all() for o in (got[0], got[1], got[3])) and (got[2] == -7).all()


# ---- the dense soft-label target -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 10])
@pytest.mark.parametrize("L", [1, 7, 3129])
def test_dense_target_equals_the_restatement_exactly(L, K):
    """Rows: all -1; labels 0 and L - 1; a duplicate label (the last one wins); labels outside [0, L) next to a real one; random.
    Twice: dense rows (ldt = L) through the Python entry point, and rows of stride L + 5 whose gap must keep its bits."""
    from vilbert import _native as N
    from vilbert import task_pipeline as tp
    rng = np.random.default_rng(L + K)
    labels = np.full((5, K), -1, dtype=np.int32)
    labels[1, 0] = 0
    labels[1, -1] = L - 1
    labels[2, :] = L // 2                                              # K > 1: K duplicates
    labels[3, 0] = L - 1
    if K > 1:
        labels[3, 1:5] = (L, -5, 2 ** 31 - 1, -2 ** 31)
    labels[4] = rng.integers(-1, L, K)
    scores = rng.uniform(0.1, 1.0, (5, K)).astype(np.float32)
    want = tr.dense_target(labels, scores, L)
    assert not want[0].any() and want[2, L // 2] == scores[2, -1] and want[3, L - 1] == scores[3, 0] and want[3].sum() == scores[3, 0]
    lab_d, sc_d = torch.from_numpy(labels).cuda(), torch.from_numpy(scores).cuda()
    same_bits(tp.dense_target(lab_d, sc_d, L).cpu().numpy(), want, "dense")
    ldt, margin = L + 5, 32
    flat = torch.full((2 * margin + 5 * ldt,), float("nan"), device="cuda")
    gap_bits = torch.arange(5 * 5, dtype=torch.float32).view(5, 5) + 0.5
    flat[margin:margin + 5 * ldt].view(5, ldt)[:, L:] = gap_bits.cuda()
    assert N.lib().vbd_dense_target(N.stream_ptr(), 5, L, K, lab_d.data_ptr(), sc_d.data_ptr(), flat[margin:].data_ptr(), ldt) == 0
    host = flat.cpu().numpy()
    body = host[margin:margin + 5 * ldt].reshape(5, ldt)
    same_bits(body[:, :L], want, "strided")
    same_bits(body[:, L:], gap_bits.numpy(), "gap")
    assert np.isnan(host[:margin]).all() and np.isnan(host[margin + 5 * ldt:]).all()


# ---- the pipeline --------------------------------------------------------------------------------------------------------------
def _task_batches(feat_dim, R, T, num_labels, seed):
    """Three batches of different N and B, the last one smaller: (source dict, expected tuple of numpy arrays)."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n_rows in enumerate(([3, R + 2, 5, 1], [R - 1, 7, R, 2, 4], [2, 6])):
        B = len(n_rows)
        batch = tr.make_packed(n_rows, feat_dim, seed=seed + i, mean_rows=[max(1, n - (j % 2)) for j, n in enumerate(n_rows)])
        lens = rng.integers(2, T + 1, B)
        batch["input_mask"] = (np.arange(T)[None] < lens[:, None]).astype(np.int64)
        batch["question"] = rng.integers(1, 90, (B, T)) * batch["input_mask"]
        batch["segment_ids"] = np.zeros((B, T), dtype=np.int64)
        batch["question_id"] = np.arange(B, dtype=np.int64) + 1000 * i
        batch["labels"] = rng.integers(-1, num_labels, (B, 4)).astype(np.int32)
        batch["scores"] = rng.uniform(0.1, 1, (B, 4)).astype(np.float32)
        batch["ref_box"] = np.concatenate([rng.uniform(0, 100, (B, 2)), rng.uniform(100, 200, (B, 2))], 1).astype(np.float32)
        out.append(batch)
    return out


def _expected(batch, R, target):
    feat, sp, mask, iou = tr.finish_task_batch(batch, R, ref_box=batch["ref_box"], iou_floor=target[1] if target[0] == "iou" else 0.0)
    tgt = tr.dense_target(batch["labels"], batch["scores"], target[1]) if target[0] == "dense" else iou
    B, T = batch["question"].shape
    return (feat, sp, mask, batch["question"], tgt, batch["input_mask"], batch["segment_ids"], np.zeros((B, R, T), np.float32),
            batch["question_id"])


@pytest.mark.parametrize("staging", ["direct", "pinned"])
@pytest.mark.parametrize("target", [("dense", 11), ("iou", 0.5)], ids=["dense", "iou"])
def test_pipeline_equals_the_restatement_batch_by_batch(staging, target):
    from vilbert import task_pipeline as tp
    R, T = 6, 9
    batches = _task_batches(16, R, T, 11, seed=40)
    assert len({b["feat"].shape[0] for b in batches}) == 3 and batches[2]["feat"].shape[0] < batches[1]["feat"].shape[0]
    pipe = tp.TaskBatchPipeline(batches, "cuda:0", R, target=target, staging=staging)
    seen, zeros = 0, {}
    for i, got in enumerate(pipe):
        want = _expected(batches[i], R, target)
        assert len(got) == 9
        for j, (g, w) in enumerate(zip(got, want)):
            same_bits(g.cpu().numpy(), w, "batch %d item %d" % (i, j))
        zeros.setdefault(tuple(got[7].shape), got[7])
        assert zeros[tuple(got[7].shape)] is got[7]                    # one cached zero tensor per shape
        torch.cuda.current_stream().synchronize()
        seen += 1
    assert seen == 3
    # the slots hold capacity: the smaller third batch went through the first slot's buffers without a reallocation
    assert pipe.slots[0].dev["feat"].shape[0] == batches[0]["feat"].shape[0] >= batches[2]["feat"].shape[0]
    assert list(zeros) == [(4, R, T), (5, R, T), (2, R, T)]


def test_pipeline_copies_a_given_target_as_it_is():
    from vilbert import task_pipeline as tp
    batches = _task_batches(8, 4, 5, 3, seed=7)
    for i, b in enumerate(batches):                                    # soft labels, then int64 class labels (cross-entropy tasks)
        ids = np.arange(len(b["question_id"]))
        b["target"] = ids.astype(np.float32)[:, None] + 0.25 if i == 0 else ids.astype(np.int64) % 3
    for i, got in enumerate(tp.TaskBatchPipeline(batches, "cuda:0", 4)):
        same_bits(got[4].cpu().numpy(), batches[i]["target"], "target %d" % i)      # same_bits compares the dtype too
        same_bits(got[0].cpu().numpy(), tr.finish_task_batch(batches[i], 4)[0], "features %d" % i)
    with pytest.raises(ValueError):
        tp.TaskBatchPipeline(batches, "cuda:0", 4, target=("sparse", 3))


def test_pipeline_batches_through_the_model_give_the_host_built_bits():
    """VILBertForVLTasks (tiny config) on what the pipeline yields and on the restatement's host-built batch: the same bits."""
    from oracle import synth
    from vilbert import task_pipeline as tp
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    cfg = synth.tiny_config()
    R, T, L = 7, 9, 13
    model = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
    model.load_state_dict(synth.make_state_dict(cfg, "vltasks"))
    model = model.eval().to("cuda:0")
    batches = _task_batches(cfg["v_feature_size"], R, T, L, seed=60)

    def forward(features, spatials, image_mask, question, target, input_mask, segment_ids, co_attention_mask, question_id):
        with torch.no_grad():
            return [o.clone() for o in model(question, features, spatials, segment_ids, input_mask, image_mask,
                                             co_attention_mask)[:9] if isinstance(o, torch.Tensor)]

    for i, got in enumerate(tp.TaskBatchPipeline(batches, "cuda:0", R, target=("dense", L))):
        out_dev = forward(*got)
        host = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in _expected(batches[i], R, ("dense", L))]
        out_host = forward(*host)
        assert len(out_dev) == len(out_host) >= 5
        for j, (a, b) in enumerate(zip(out_dev, out_host)):
            assert a.shape == b.shape and torch.equal(a, b), (i, j)         # (a NaN would not equal itself)


# ---- graph capture -------------------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_eager_bits():
    from vilbert import task_pipeline as tp
    batch = _task_batches(64, 12, 6, 50, seed=80)[1]
    dev = _to_dev({k: batch[k] for k in tp.PACKED_FIELDS})
    ref_box, labels, scores = (torch.from_numpy(batch[n]).cuda() for n in ("ref_box", "labels", "scores"))

    def run():
        return tp.finish_task_batch(dev, 12, ref_box=ref_box, iou_floor=0.5) + (tp.dense_target(labels, scores, 50),)

    eager = run()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    for t in captured:
        t.fill_(-7)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    want = tr.finish_task_batch(batch, 12, ref_box=batch["ref_box"], iou_floor=0.5) + (tr.dense_target(batch["labels"], batch["scores"], 50),)
    for c, e, w in zip(captured, eager, want):
        assert torch.equal(c, e)
        same_bits(c.cpu().numpy(), w, "replayed")
