"""The device-resident region store on the GPU (csrc/region_store.hip, vilbert.region_store): a batch gathered by image index
equals, bit for bit, what the packed builder (vilbert.task_pipeline.finish_task_batch, itself pinned to the reference's recorded
outputs by tests/test_task_batch_gpu.py) gives for ``pack_task_samples`` of the same images - the work is copies, zeros, an fp32
sum in row order and single correctly rounded fp32 operations by the SAME kernels, so there is no tolerance anywhere in this
file. Invalid ids and corrupt store words are held to the numpy restatement (tests/region_store_restatement.py)."""
import ctypes

import numpy as np
import pytest
import torch

import region_store_restatement as rr
from test_region_store import ID_LISTS, STORE_MEANS, STORE_ROWS, store_arrays, store_samples
from test_task_batch import same_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT_NAMES = ("features", "spatials", "image_mask", "target")
KINDS = {"f32": (np.float32, torch.float32, torch.float32), "f16": (np.float16, torch.float16, torch.float32),
         "f16_bf16": (np.float16, torch.float16, torch.bfloat16)}


def _to_dev(packed):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in packed.items() if v is not None}


def _bits(t):
    """Raw words of a tensor: bf16 and fp32 blocks are compared as integers (a NaN equals itself, -0 differs from +0)."""
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _equal(got, want, what):
    assert len(got) == len(want), what
    for g, w, name in zip(got, want, OUT_NAMES):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert torch.equal(_bits(g), _bits(w)), (what, name)


def _store(samples, torch_dtype, means=None, split=3):
    """The test store, added in two chunks so that the second one's offsets are rebased."""
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    np_dtype = np.float16 if torch_dtype == torch.float16 else np.float32
    store = rs.RegionStore(DEV, sum(STORE_ROWS), len(STORE_ROWS), feat_dim=samples[0]["feat"].shape[1], dtype=torch_dtype,
                           with_mean_rows=means is not None)
    first = store.add(tp.pack_task_samples(samples[:split], mean_rows=None if means is None else means[:split], dtype=np_dtype))
    second = store.add(tp.pack_task_samples(samples[split:], mean_rows=None if means is None else means[split:], dtype=np_dtype))
    assert (first, second) == (range(0, split), range(split, len(samples)))
    assert (store.num_images, store.total_rows) == (len(STORE_ROWS), sum(STORE_ROWS))
    return store


def _packed_reference(samples, ids, means, R, np_dtype, out_dtype, ref_box=None, iou_floor=0.0):
    from vilbert import task_pipeline as tp
    packed = tp.pack_task_samples([samples[i] for i in ids], mean_rows=None if means is None else [means[i] for i in ids],
                                  dtype=np_dtype)
    if means is None:
        packed["mean_rows"] = None
    return tp.finish_task_batch(_to_dev(packed), R, ref_box=ref_box, iou_floor=iou_floor, out_dtype=out_dtype)


# ---- the grid --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("F", [8, 264, 520, 2048])
def test_gathered_batches_equal_the_packed_builder_exactly(F, kind):
    """F: the smallest column group, more than one block in x for fp32 (256 columns a block) and for binary16 (512), the real
    width. R = 1 keeps only the mean row; the id lists repeat and permute images; mean_rows absent and present."""
    np_dtype, store_dtype, out_dtype = KINDS[kind]
    samples = store_samples(F, np_dtype, seed=F)
    ascending = torch.tensor(ID_LISTS["ascending"], dtype=torch.int64, device=DEV)
    for means in (None, STORE_MEANS):
        store = _store(samples, store_dtype, means)
        assert store.feat.dtype == store_dtype and store.nbytes > 0
        same_bits(store.image_offsets.cpu().numpy(), np.concatenate([[0], np.cumsum(STORE_ROWS)]).astype(np.int64), "rebased offsets")
        for R in (1, 2, 9, 37):
            for name, ids in sorted(ID_LISTS.items()):
                want = _packed_reference(samples, ids, means, R, np_dtype, out_dtype)
                got = store.batch(ids, R, out_dtype=out_dtype)                         # host ids: validated, uploaded
                assert got[0].dtype == out_dtype and got[2].sum(1).tolist() == [min(STORE_ROWS[i] + 1, R) for i in ids]
                _equal(got, want, "%s R=%d mean=%s" % (name, R, means is not None))
            want = _packed_reference(samples, ID_LISTS["ascending"], means, R, np_dtype, out_dtype)
            _equal(store.batch(ascending, R, out_dtype=out_dtype), want, "device ids R=%d" % R)     # a device tensor: used as it is


@pytest.mark.parametrize("floor", [0.0, 0.5])
def test_iou_target_uses_the_box_of_the_batch_row_not_of_the_image(floor):
    samples = store_samples(8, np.float32)
    store = _store(samples, torch.float32, STORE_MEANS)
    ids = ID_LISTS["permuted"]
    wh = np.array([[samples[i]["image_w"], samples[i]["image_h"]] for i in ids], dtype=np.float32)
    rng = np.random.default_rng(3)
    lo = rng.uniform(0, 0.5, (len(ids), 2)) * wh
    ref_box = np.concatenate([lo, lo + rng.uniform(0.2, 0.5, (len(ids), 2)) * wh], 1).astype(np.float32)
    for b in (0, 4):                                                   # a reference box that IS a kept region: IoU 1 survives the floor
        ref_box[b] = samples[ids[b]]["boxes"][0]
    assert ids[1] == ids[2] and not np.array_equal(ref_box[1], ref_box[2])
    rb = torch.from_numpy(ref_box).to(DEV)
    want = _packed_reference(samples, ids, STORE_MEANS, 37, np.float32, torch.float32, ref_box=rb, iou_floor=floor)
    got = store.batch(ids, 37, ref_box=rb, iou_floor=floor)
    _equal(got, want, "iou")
    assert len(got) == 4 and torch.equal(got[0][1], got[0][2]) and got[3][0, 1, 0] == 1 and got[3][4, 1, 0] == 1
    if floor == 0.0:
        assert not torch.equal(got[3][1], got[3][2]) and ((got[3] > 0) & (got[3] < 0.5)).any()
    else:
        assert not ((got[3] > 0) & (got[3] < 0.5)).any()
    for g, w, name in zip(got, rr.finish_store_batch(store_arrays(samples, STORE_MEANS), ids, 37, ref_box=ref_box, iou_floor=floor),
                          OUT_NAMES):
        same_bits(g.cpu().numpy(), w, "restatement " + name)


# ---- ids and store words nobody validated ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_invalid_device_ids_give_padding_and_leave_their_neighbours_alone(kind):
    np_dtype, store_dtype, out_dtype = KINDS[kind]
    samples = store_samples(24, np_dtype)
    store = _store(samples, store_dtype, STORE_MEANS)
    ids = torch.tensor([-1, 3, len(STORE_ROWS), 2 ** 40, 0], dtype=torch.int64, device=DEV)
    rb = torch.tensor([[10, 10, 150, 150]] * 5, dtype=torch.float32, device=DEV)
    got = store.batch(ids, 12, ref_box=rb, out_dtype=out_dtype)
    want = _packed_reference(samples, [3, 0], STORE_MEANS, 12, np_dtype, out_dtype, ref_box=rb[:2])
    for g, w, name in zip(got, want, OUT_NAMES):
        assert not _bits(g[[0, 2, 3]]).any(), name                     # every word +0: features, spatials, mask, target
        assert torch.equal(_bits(g[[1, 4]]), _bits(w)), name
    assert got[2][:, 0].tolist() == [0, 1, 0, 0, 1]                    # how a caller sees an invalid id


def _native_store_call(store, ids, R, ref_box=None, iou_floor=0.0, guard=16):
    """vbr_store_finish_batch through the C ABI on `store` (numpy arrays, as the restatement takes them) laid out on the device
    between guard bands: `guard` rows of NaN (features, boxes) and words of a huge offset / size / count (image words) before
    and after each store array. Outputs are pre-filled with NaN (the mask with -7). Returns (code, outputs, unchanged) where
    unchanged says that every store array and its guard bands still hold what was uploaded."""
    from vilbert import _native as N
    feat, boxes = store["feat"], store["boxes"]
    n, F, I, B = feat.shape[0], feat.shape[1], len(store["image_offsets"]) - 1, len(ids)
    bands = dict(feat=np.concatenate([np.full((guard, F), np.nan, feat.dtype), feat, np.full((guard, F), np.nan, feat.dtype)]),
                 boxes=np.concatenate([np.full((guard, 4), np.nan, np.float32), boxes, np.full((guard, 4), np.nan, np.float32)]),
                 image_offsets=np.concatenate([np.full(guard, 2 ** 50, np.int64), store["image_offsets"], np.full(guard, 2 ** 50, np.int64)]),
                 image_wh=np.concatenate([np.full((guard, 2), -9, np.int32), store["image_wh"], np.full((guard, 2), -9, np.int32)]))
    if store.get("mean_rows") is not None:
        bands["mean_rows"] = np.concatenate([np.full(guard, 2 ** 30, np.int32), store["mean_rows"], np.full(guard, 2 ** 30, np.int32)])
    dev = _to_dev(bands)
    a = N.StoreBatchArgs()
    a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.total_rows, a.num_images = B, R, F, iou_floor, n, I
    a.feat_kind, a.out_kind = (1 if feat.dtype == np.float16 else 0), 0
    for name in bands:
        setattr(a, name, dev[name][guard:].data_ptr())
    ids_dev = torch.tensor(list(ids), dtype=torch.int64, device=DEV)
    a.image_ids = ids_dev.data_ptr()
    outs = [torch.full(s, float("nan"), device=DEV) for s in ((B, R, F), (B, R, 5))] + \
           [torch.full((B, R), -7, dtype=torch.int64, device=DEV), torch.full((B, R, 1), float("nan"), device=DEV)]
    a.out_feat, a.out_spatials, a.out_mask = (o.data_ptr() for o in outs[:3])
    if ref_box is not None:
        rb = torch.from_numpy(np.asarray(ref_box, dtype=np.float32)).to(DEV)
        a.ref_box, a.out_iou = rb.data_ptr(), outs[3].data_ptr()
    code = N.lib().vbr_store_finish_batch(N.stream_ptr(), ctypes.byref(a))
    torch.cuda.synchronize()
    unchanged = all(np.array_equal(dev[name].cpu().numpy().view(np.uint8), np.ascontiguousarray(bands[name]).view(np.uint8))
                    for name in bands)
    return code, [o.cpu().numpy() for o in outs[:4 if ref_box is not None else 3]], unchanged


@pytest.mark.parametrize("np_dtype", [np.float32, np.float16], ids=["f32", "f16"])
def test_corrupt_store_words_are_clamped_before_any_address_is_formed(np_dtype):
    """A decreasing offset, an offset past total_rows (the rows beyond it are guard rows of NaN: one of them read would show in
    the outputs) and a mean_rows beyond the image's count. The outputs equal the restatement, which states the clamps."""
    samples = store_samples(16, np_dtype)
    good = store_arrays(samples, STORE_MEANS)
    ids = [6, 0, 0, 7, 3, 2, 2, 5, 4, 1]
    ref_box = np.tile(np.array([[20, 20, 180, 180]], np.float32), (len(ids), 1))
    code, got, unchanged = _native_store_call(good, ids, 9, ref_box=ref_box)          # the helper on a healthy store first
    assert code == 0 and unchanged
    for g, w, name in zip(got, rr.finish_store_batch(good, ids, 9, ref_box=ref_box), OUT_NAMES):
        same_bits(g, w, "healthy " + name)
    bad = dict(good, image_offsets=good["image_offsets"].copy(), mean_rows=good["mean_rows"].copy())
    total = int(good["image_offsets"][-1])
    bad["image_offsets"][3] = bad["image_offsets"][2] - 2              # decreasing: image 2 owns nothing, image 3 starts early
    bad["image_offsets"][7] = total + 5                                # past total_rows: image 6 runs into the end, image 7 is empty
    bad["image_offsets"][8] = total + 9
    bad["mean_rows"][4], bad["mean_rows"][1] = 2 ** 20, -3             # beyond the count; negative
    for R in (9, 120):                                                 # 120: nothing truncates image 6's clamped rows
        code, got, unchanged = _native_store_call(bad, ids, R, ref_box=ref_box)
        assert code == 0 and unchanged
        want = rr.finish_store_batch(bad, ids, R, ref_box=ref_box)
        assert want[2].sum(1).tolist() == [min(R, n) for n in (total - 40 + 1, 2, 2, 1, 20, 1, 1, 3, 18, 4)]
        for g, w, name in zip(got, want, OUT_NAMES):
            same_bits(g, w, "corrupt R=%d %s" % (R, name))             # (a NaN read from a guard row would differ)


def test_empty_batch():
    store = _store(store_samples(8, np.float16), torch.float16)
    for ids in (torch.empty(0, dtype=torch.int64, device=DEV), []):
        out = store.batch(ids, 5, ref_box=torch.empty(0, 4, device=DEV), out_dtype=torch.bfloat16)
        assert [tuple(o.shape) for o in out] == [(0, 5, 8), (0, 5, 5), (0, 5), (0, 5, 1)] and out[0].dtype == torch.bfloat16
    torch.cuda.synchronize()


# ---- element offsets beyond 32 bits ----------------------------------------------------------------------------------------------
def test_rows_beyond_2_to_31_elements():
    """A binary16 store of 2^20 + 64 rows of 2048 columns (4.3 GB, left uninitialised but for the rows that are read): the last
    two images start at element 2^31. Through the C ABI, against the packed builder on the same rows as slices."""
    from vilbert import _native as N
    from vilbert import task_pipeline as tp
    free = torch.cuda.mem_get_info()[0]
    if free < 6 * 2 ** 30:
        pytest.skip("needs 6 GB of free device memory for the 4.3 GB store, %.1f GB are free" % (free / 2 ** 30))
    big, F = 2 ** 20, 2048
    rows = big + 64
    feat = torch.empty(rows, F, dtype=torch.float16, device=DEV)
    boxes = torch.empty(rows, 4, dtype=torch.float32, device=DEV)
    p = store_samples(F, np.float16, seed=5)[6]                        # 100 rows of values: 64 for the tail, 2 for the head
    feat[big:].copy_(torch.from_numpy(p["feat"][:64]))
    boxes[big:].copy_(torch.from_numpy(p["boxes"][:64]))
    feat[:2].copy_(torch.from_numpy(p["feat"][64:66]))                 # the only rows of image 0 that its batch reads
    boxes[:2].copy_(torch.from_numpy(p["boxes"][64:66]))
    offsets = torch.tensor([0, big, big + 41, rows], dtype=torch.int64, device=DEV)
    wh = torch.tensor([[640, 480], [500, 375], [333, 500]], dtype=torch.int32, device=DEV)
    mean = torch.tensor([2, 41, 7], dtype=torch.int32, device=DEV)
    assert big * F == 2 ** 31

    def gather(ids, R):
        a = N.StoreBatchArgs()
        a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.feat_kind, a.out_kind = len(ids), R, F, 0.0, 1, 0
        a.total_rows, a.num_images = rows, 3
        a.feat, a.boxes, a.image_offsets, a.image_wh, a.mean_rows = (t.data_ptr() for t in (feat, boxes, offsets, wh, mean))
        ids_dev = torch.tensor(ids, dtype=torch.int64, device=DEV)
        a.image_ids = ids_dev.data_ptr()
        outs = (torch.full((len(ids), R, F), float("nan"), device=DEV), torch.full((len(ids), R, 5), float("nan"), device=DEV),
                torch.full((len(ids), R), -7, dtype=torch.int64, device=DEV))
        a.out_feat, a.out_spatials, a.out_mask = (o.data_ptr() for o in outs)
        assert N.lib().vbr_store_finish_batch(N.stream_ptr(), ctypes.byref(a)) == 0
        torch.cuda.synchronize()
        return outs

    # the packed builder takes its samples back to back: image 2 (rows big + 41 ..) and image 1 (rows big ..) one at a time
    got = gather([2, 1], 45)
    for b, (lo, hi, img) in enumerate(((big + 41, rows, 2), (big, big + 41, 1))):
        one = dict(feat=feat[lo:hi], boxes=boxes[lo:hi], offsets=torch.tensor([0, hi - lo], dtype=torch.int64, device=DEV),
                   image_wh=wh[img:img + 1], mean_rows=mean[img:img + 1])
        want = tp.finish_task_batch(one, 45)
        _equal([g[b:b + 1] for g in got], want, "image %d" % img)
    assert got[2].sum(1).tolist() == [24, 42]
    # image 0 owns 2^20 rows; R = 3 and mean_rows = 2 keep its batch to the two leading rows
    head = dict(feat=feat[:2], boxes=boxes[:2], offsets=torch.tensor([0, 2], dtype=torch.int64, device=DEV), image_wh=wh[:1],
                mean_rows=mean[:1])
    _equal(gather([0], 3), tp.finish_task_batch(head, 3), "image 0")


# ---- graph capture ---------------------------------------------------------------------------------------------------------------
def test_graph_replay_on_new_ids_gives_the_eager_bits():
    samples = store_samples(64, np.float16)
    store = _store(samples, torch.float16, STORE_MEANS)
    first, second = [6, 0, 0, 7, 3, 2, 2, 5], [1, 1, 4, -1, 6, 5, 3, 0]
    ids_dev = torch.tensor(first, dtype=torch.int64, device=DEV)
    rb = torch.tensor([[5, 5, 120, 140]] * 8, dtype=torch.float32, device=DEV)

    def run():
        return store.batch(ids_dev, 12, ref_box=rb, iou_floor=0.5, out_dtype=torch.bfloat16)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run()
    graph.replay()
    torch.cuda.synchronize()
    _equal(captured, run(), "replay on the captured ids")
    ids_dev.copy_(torch.tensor(second, dtype=torch.int64))             # in place: the graph reads the same address
    for t in captured:
        t.fill_(-7)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    eager = store.batch(torch.tensor(second, dtype=torch.int64, device=DEV), 12, ref_box=rb, iou_floor=0.5, out_dtype=torch.bfloat16)
    _equal(captured, eager, "replay on new ids")
    assert captured[2][:, 0].tolist() == [1, 1, 1, 0, 1, 1, 1, 1]


# ---- the pipeline ----------------------------------------------------------------------------------------------------------------
def _id_batches(T, num_labels, seed=40):
    """Three batches of sizes 4 / 4 / 2 as a source of StoreBatchPipeline yields them: image ids (repeated, permuted), token
    arrays and the inputs of every target kind."""
    rng = np.random.default_rng(seed)
    out = []
    for i, ids in enumerate(([6, 0, 0, 7], [3, 2, 2, 5], [4, 1])):
        B = len(ids)
        lens = rng.integers(2, T + 1, B)
        mask = (np.arange(T)[None] < lens[:, None]).astype(np.int64)
        out.append(dict(image_ids=np.array(ids), input_mask=mask, question=rng.integers(1, 90, (B, T)) * mask,
                        segment_ids=np.zeros((B, T), dtype=np.int64), question_id=np.arange(B, dtype=np.int64) + 1000 * i,
                        labels=rng.integers(-1, num_labels, (B, 4)).astype(np.int32),
                        scores=rng.uniform(0.1, 1, (B, 4)).astype(np.float32),
                        target=(np.arange(B) % 3).astype(np.int64),
                        ref_box=np.concatenate([rng.uniform(0, 100, (B, 2)), rng.uniform(100, 200, (B, 2))], 1).astype(np.float32)))
    return out


def _packed_batches(id_batches, samples, means, np_dtype):
    from vilbert import task_pipeline as tp
    out = []
    for b in id_batches:
        ids = b["image_ids"].tolist()
        packed = tp.pack_task_samples([samples[i] for i in ids], mean_rows=[means[i] for i in ids], dtype=np_dtype)
        out.append(dict({k: v for k, v in b.items() if k != "image_ids"}, **packed))
    return out


@pytest.mark.parametrize("kind", ["f32", "f16_bf16"])
@pytest.mark.parametrize("target", [None, ("dense", 11), ("iou", 0.5)], ids=["given", "dense", "iou"])
def test_store_pipeline_equals_the_packed_pipeline_element_for_element(target, kind):
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    np_dtype, store_dtype, out_dtype = KINDS[kind]
    samples = store_samples(16, np_dtype)
    store = _store(samples, store_dtype, STORE_MEANS)
    id_batches = _id_batches(9, 11)
    packed = tp.TaskBatchPipeline(_packed_batches(id_batches, samples, STORE_MEANS, np_dtype), DEV, 6, target=target,
                                  wire_dtype=torch.float16 if np_dtype == np.float16 else None, feature_dtype=out_dtype)
    stored = rs.StoreBatchPipeline(id_batches, store, 6, target=target, feature_dtype=out_dtype)
    seen = 0
    for got, want in zip(stored, packed):
        assert len(got) == len(want) == 9 and got[0].dtype == out_dtype
        for j, (g, w) in enumerate(zip(got, want)):
            assert g.shape == w.shape and g.dtype == w.dtype and torch.equal(_bits(g), _bits(w)), (seen, j)
        assert got[0].shape[0] == (4, 4, 2)[seen]
        torch.cuda.current_stream().synchronize()
        seen += 1
    assert seen == 3
    assert sorted(stored.slots[0].dev) == sorted(stored.fields) and "feat" not in stored.slots[0].dev      # nothing packed travelled


def test_store_batches_through_the_model_give_the_packed_batches_loss_and_gradients():
    """VILBertForVLTasks (tiny config), one forward + backward per pipeline: identical loss and gradient bits."""
    import vilbert.vilbert as V
    from oracle import synth
    from vilbert import _native
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    from vilbert.vilbert import BertConfig, VILBertForVLTasks
    cfg = synth.tiny_config()
    R, T = 7, 9
    samples = store_samples(cfg["v_feature_size"], np.float32)
    store = _store(samples, torch.float32, STORE_MEANS)
    id_batches = _id_batches(T, 13)[:1]
    model = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1)
    model.load_state_dict(synth.make_state_dict(cfg, "vltasks"))
    model = model.to(DEV).train()

    def step(features, spatials, image_mask, question, target, input_mask, segment_ids, co_attention_mask, question_id):
        model.zero_grad(set_to_none=True)
        out = model(question, features, spatials, segment_ids, input_mask, image_mask, co_attention_mask)[:9]
        loss = sum(o.float().mean() for i, o in enumerate(out) if i != 6 and isinstance(o, torch.Tensor) and o.requires_grad)
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    wanted = _native._DET["wanted"]
    _native.set_deterministic(True)
    orig, V._drop_p = V._drop_p, (lambda m: 0.0)
    try:
        results = [step(*next(iter(pipe))) for pipe in
                   (rs.StoreBatchPipeline(id_batches, store, R, target=("dense", 13)),
                    tp.TaskBatchPipeline(_packed_batches(id_batches, samples, STORE_MEANS, np.float32), DEV, R, target=("dense", 13)))]
    finally:
        V._drop_p = orig
        _native.set_deterministic(wanted)
    (loss_s, grads_s), (loss_p, grads_p) = results
    assert torch.equal(loss_s, loss_p) and torch.isfinite(loss_s)
    assert grads_s.keys() == grads_p.keys() and len(grads_s) > 20
    for n in grads_s:
        assert torch.equal(_bits(grads_s[n]), _bits(grads_p[n])), n
    assert any(g.abs().sum() > 0 for n, g in grads_s.items() if "v_embeddings" in n)         # the features reached the loss
