"""The half-width (float16) feature wire on the GPU (csrc/feat_rows.h, batch.hip, task_batch.hip, wire16.hip; vilbert.input_pipeline
/ vilbert.task_pipeline with float16 features; BertImageEmbeddings with a bf16 feature block). The yardstick is the fp32 path run
on the exactly widened arrays and - most of the two being instantiations of one kernel template - the numpy restatements of
both calls (section 4b); every comparison is torch.equal: widening binary16 is exact, the sums run in the same order, the bf16
output is one correctly rounded conversion of the fp32 result. There is no tolerance anywhere in this file."""
import ctypes

import numpy as np
import pytest
import torch

import masking_restatement as mr
import task_batch_restatement as tr
import wire16_cases as wc
from oracle import batch_oracle as bo
from oracle import synth
from test_task_batch import GOLDEN, golden_refer_batch, golden_sample

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _to_dev(raw):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in raw.items() if v is not None}


def _same(got, want, name):
    """Same shape, dtype and values; a float tensor that may hold NaN is compared through its bits by the callers."""
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    assert torch.equal(got, want), name


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _round_bf16(t):
    """fp32 device tensor -> bf16, rounded to nearest even on the HOST by torch's CPU cast."""
    return t.cpu().to(torch.bfloat16)


# ---- 1, 2: Conceptual-Captions finishing ---------------------------------------------------------------------------------------
_CONCAP = {}


def _concap_case(F):
    """B = 3, R = 5, T = 6 with float16 features; sample 1 has every masked_label != 0 (the count falls back to 1). Returns the
    float16 raw dict and, per objective, what the fp32 path gives on the widened features (computed once, left unchanged)."""
    if F not in _CONCAP:
        raw = bo.make_raw_batch(3, tokens=6, regions=5, feat_dim=F, n_classes=9, vocab=99, seed=F)
        raw["masked_label"][1] = 1
        raw["masked_label"][0, :2] = 0
        half = dict(raw, image_feat=wc.f16_values((3, 5, F), F))
        wide = dict(raw, image_feat=wc.widen(half["image_feat"]))
        from vilbert import input_pipeline as ip
        want = {obj: ip.finish_batch(_to_dev(wide), obj) for obj in (0, 1)}
        torch.cuda.synchronize()
        _CONCAP[F] = (half, want)
    return _CONCAP[F]


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("F", [8, 264, 2048])
def test_concap_finishing_equals_the_fp32_path_on_the_widened_features(F, objective):
    """F = 8: one 16-byte group; F = 264: 33 groups, a partial block; F = 2048: the real width, four blocks per sample."""
    from vilbert import input_pipeline as ip
    half, want = _concap_case(F)
    dev = _to_dev(half)
    got = ip.finish_batch(dev, objective)
    assert len(got) == 10 and got[5].dtype == torch.float32
    for j in range(10):
        _same(got[j], want[objective][j], "fp32 out, item %d" % j)
    _same(dev["image_feat"].cpu(), torch.from_numpy(half["image_feat"]), "the float16 input")        # only read
    # the mean row of the sample whose count falls back to 1 is the plain sum
    if objective == 0:
        s = np.zeros(F, np.float32)
        for r in range(5):
            s = s + wc.widen(half["image_feat"][1, r])
        assert np.array_equal(got[5][1, 0].cpu().numpy(), s)


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("F", [8, 264, 2048])
def test_concap_bf16_output_is_the_rounded_fp32_result(F, objective):
    from vilbert import input_pipeline as ip
    half, want = _concap_case(F)
    got = ip.finish_batch(_to_dev(half), objective, out_dtype=torch.bfloat16)
    assert got[5].dtype == torch.bfloat16
    _same(got[5].cpu(), _round_bf16(want[objective][5]), "bf16 features")
    for j in (0, 1, 2, 3, 4, 6, 7, 8, 9):
        _same(got[j], want[objective][j], "bf16 out, item %d" % j)


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_concap_infinity_and_nan_pass_through(out_dtype):
    from vilbert import input_pipeline as ip
    half, _ = _concap_case(8)
    feat = half["image_feat"].copy()
    feat[0, 2, 3], feat[2, 4, 6] = np.float16(np.inf), np.float16(np.nan)
    feat[0, :, 3][[0, 1, 3, 4]] = np.float16(1.5)                              # finite neighbours: the column sum is +Inf
    dev = _to_dev(dict(half, image_feat=feat))
    got = ip.finish_batch(dev, 0, out_dtype=out_dtype)[5].float().cpu()
    want = ip.finish_batch(_to_dev(dict(half, image_feat=wc.widen(feat))), 0)[5].cpu()
    assert got[0, 3, 3] == float("inf") and got[0, 0, 3] == float("inf")       # the row element and the mean column
    assert torch.isnan(got[2, 5, 6]) and torch.isnan(got[2, 0, 6])
    assert int(torch.isnan(got).sum()) == 2 and int(torch.isinf(got).sum()) == 2
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    finite = ~torch.isnan(want)
    want = want if out_dtype == torch.float32 else want.to(torch.bfloat16).float()
    assert torch.equal(got[finite], want[finite])


def test_concap_outputs_are_written_completely_and_nothing_else_is():
    """The C ABI straight: NaN-filled outputs between canary margins, F = 264 (a partial block), both output kinds."""
    from vilbert import _native as N
    from vilbert import input_pipeline as ip
    half, want = _concap_case(264)
    dev = _to_dev(half)
    B, R, T, F, margin = 3, 5, 6, 264, 64
    for kind, dt in ((0, torch.float32), (1, torch.bfloat16)):
        flat = torch.full((2 * margin + B * (R + 1) * F,), float("nan"), dtype=dt, device=DEV)
        loc = torch.full((B, R + 1, 5), float("nan"), device=DEV)
        mask, ilab, lm = (torch.full(s, -7, dtype=torch.int64, device=DEV) for s in ((B, R + 1), (B, R), (B, T)))
        a = N.WireConcapBatch()
        a.batch, a.regions, a.tokens, a.feat_dim, a.objective, a.out_kind = B, R, T, F, 0, kind
        for n in ("image_feat", "image_loc", "image_mask", "masked_label", "is_next", "image_label", "lm_label_ids"):
            setattr(a, n, dev[n].data_ptr())
        a.out_image_feat, a.out_image_loc = flat[margin:].data_ptr(), loc.data_ptr()
        a.out_image_mask, a.out_image_label, a.out_lm_label_ids = mask.data_ptr(), ilab.data_ptr(), lm.data_ptr()
        assert N.lib().vbw_concap_finish_batch(N.stream_ptr(), ctypes.byref(a)) == 0
        torch.cuda.synchronize()
        host = flat.cpu()
        assert torch.isnan(host[:margin]).all() and torch.isnan(host[margin + B * (R + 1) * F:]).all(), "a canary margin was written"
        body = host[margin:margin + B * (R + 1) * F].view(B, R + 1, F)
        _same(body, want[0][5].cpu() if kind == 0 else _round_bf16(want[0][5]), "features, kind %d" % kind)
        for g, j in ((loc, 6), (mask, 9), (ilab, 8), (lm, 3)):
            _same(g, want[0][j], "item %d" % j)
    assert N.lib().vbw_concap_finish_batch(N.stream_ptr(), None) == -1


# ---- 3: fused row clearing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "copy"])
def test_masking_then_finishing_on_float16_equals_the_fp32_path_and_never_writes_the_features(inplace):
    from vilbert import input_pipeline as ip
    c = wc.MASK_CASE
    raw, feat = wc.mask_case_raw()
    wide_dev = _to_dev(raw)
    masked = ip.mask_batch(wide_dev, c["seed"], wc.VOCAB, wc.MASK_ID, c["p"], inplace=False)
    want = ip.finish_batch(masked, 0)
    half_dev = _to_dev(dict(raw, image_feat=feat))
    got_masked = ip.mask_batch(half_dev, c["seed"], wc.VOCAB, wc.MASK_ID, c["p"], inplace=inplace)
    assert sorted(got_masked) == sorted(ip.RAW_FIELDS + ("zero_row",))
    assert got_masked["image_feat"] is half_dev["image_feat"] and got_masked["zero_row"].dtype == torch.uint8
    _same(got_masked["zero_row"].cpu(), torch.from_numpy(wc.mask_case_flags(raw)), "zero_row")
    for n in ("input_ids", "lm_label_ids", "image_label", "masked_label"):
        _same(got_masked[n], masked[n], "masked " + n)
    got = ip.finish_batch(got_masked, 0)
    for j in range(10):                                                        # all ten outputs
        _same(got[j], want[j], "item %d" % j)
    flags = got_masked["zero_row"].bool()
    assert flags.any() and not got[5][:, 1:][flags].any()                      # the flagged rows are zeros
    _same(_bits(half_dev["image_feat"]).cpu(), torch.from_numpy(feat.view(np.int16)), "the float16 buffer afterwards")
    got16 = ip.finish_batch(got_masked, 0, out_dtype=torch.bfloat16)
    _same(got16[5].cpu(), _round_bf16(want[5]), "bf16 features")


# ---- 4: the fine-tuning builder ------------------------------------------------------------------------------------------------
def _narrow_packed(packed, seed):
    """The packed batch with float16 features of the same shape (full-mantissa values), and its exactly widened twin."""
    half = dict(packed, feat=wc.f16_values(packed["feat"].shape, seed))
    return half, dict(packed, feat=wc.widen(half["feat"]))


def _check_task(half, wide, R, ref_box=None, iou_floor=0.0):
    from vilbert import task_pipeline as tp
    rb = None if ref_box is None else torch.from_numpy(np.asarray(ref_box, dtype=np.float32)).to(DEV)
    want = tp.finish_task_batch(_to_dev(wide), R, ref_box=rb, iou_floor=iou_floor)
    dev = _to_dev(half)
    got = tp.finish_task_batch(dev, R, ref_box=rb, iou_floor=iou_floor)
    got16 = tp.finish_task_batch(dev, R, ref_box=rb, iou_floor=iou_floor, out_dtype=torch.bfloat16)
    assert len(got) == len(got16) == len(want) == (3 if ref_box is None else 4)
    for j, w in enumerate(want):
        _same(got[j], w, "fp32 out, item %d" % j)
        _same(got16[j].cpu(), _round_bf16(w) if j == 0 else w.cpu(), "bf16 out, item %d" % j)
    assert got16[0].dtype == torch.bfloat16
    return want


def test_task_builder_on_the_golden_images_narrowed_to_float16():
    """Regions 3 / 5 / 6 / 9 against max_regions = 6 (below, at and above the cut), F = 2048: the plain target-less batch and
    the refer-expression batches (IoU target, floor 0 and 0.5, ground-truth rows that stay out of the mean)."""
    from vilbert import task_pipeline as tp
    g = dict(np.load(GOLDEN))
    R = int(g["max_regions"])
    assert R == 6 and {3, 5, 6, 9} <= {int(n) for n in g["img_rows"]}
    packed = tp.pack_task_samples([golden_sample(g, i) for i in g["vqa_image"]])
    half, wide = _narrow_packed(packed, 1)
    want = _check_task(half, wide, R)
    kept = want[2].sum(1).cpu().tolist()
    assert min(kept) < R and max(kept) == R
    for split, floor in (("val", 0.0), ("train", 0.5)):
        packed, ref_box, split_floor, _ = golden_refer_batch(g, split)
        assert split_floor == floor
        half, wide = _narrow_packed(packed, 2)
        want = _check_task(half, wide, R, ref_box, floor)
        assert (want[3] > 0).any()


@pytest.mark.parametrize("floor", [0.0, 0.5])
def test_task_builder_small_width_partial_means_and_an_empty_sample(floor):
    """F = 8 (one 16-byte group per row): mean_rows below the row count, more rows than R keeps, 9 rows through the unrolled
    loop's second group, and offsets that clamp a sample to nothing (its mean row is zeros, its other rows padding)."""
    packed = tr.make_packed([4, 9, 1, 6], 8, seed=11, mean_rows=[2, 7, 1, 6])
    packed["offsets"] = np.array([0, 4, 13, 13, 20], dtype=np.int64)           # sample 2: empty; sample 3: rows 13 .. 19
    packed["mean_rows"] = np.array([2, 7, 1, 6], dtype=np.int32)               # (clamped to 0 for the empty sample)
    half, wide = _narrow_packed(packed, 3)
    ref = np.array([[10, 10, 60, 60]] * 4, dtype=np.float32)
    for R in (1, 6):
        want = _check_task(half, wide, R, ref, floor)
        assert want[2].sum(1).cpu().tolist() == [min(5, R), min(10, R), 1, min(8, R)]
        assert not want[0][2].any()
    half.pop("mean_rows"), wide.pop("mean_rows")                               # NULL: all rows enter the mean
    _check_task(half, wide, 6)
    half["mean_rows"] = wide["mean_rows"] = None
    _check_task(half, wide, 12)                                                # zero rows behind every sample


# ---- 4b: host yardsticks -------------------------------------------------------------------------------------------------------
# The float16 kernels and the fp32 task builder are instantiations of ONE kernel template (csrc/feat_rows.h), so the comparisons
# above partly hold one instantiation to another. These hold every feature kernel to a numpy restatement that shares no code
# with the library (the fp32 task builder: tests/test_task_batch_gpu.py).
_ORACLE = {}


def _concap_oracle(F, R, half):
    """(raw dict as the call takes it, {objective: oracle output}) for B = 3, T = 6; sample 0 has no masked_label == 0 (the
    count falls back to 1). half: float16 features with full mantissas, the oracle runs on their exact widening."""
    key = (F, R, half)
    if key not in _ORACLE:
        raw = bo.make_raw_batch(3, tokens=6, regions=R, feat_dim=F, n_classes=9, vocab=99, seed=F + R)
        assert (raw["masked_label"][0] != 0).all() and (raw["masked_label"][1:] == 0).any()
        wide = raw
        if half:
            raw = dict(raw, image_feat=wc.f16_values((3, R, F), F + R))
            wide = dict(raw, image_feat=wc.widen(raw["image_feat"]))
        _ORACLE[key] = (raw, {obj: bo.finish_batch(wide, obj) for obj in (0, 1)})
    return _ORACLE[key]


def _equals_oracle(got, want, bf16=False):
    assert len(got) == len(bo.OUT_FIELDS)
    for g, name in zip(got, bo.OUT_FIELDS):
        w = torch.from_numpy(np.ascontiguousarray(want[name]))
        if bf16 and name == "image_feat":
            w = w.to(torch.bfloat16)                       # torch's CPU cast: round to nearest even
        _same(g.cpu(), w, name)


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("R", [3, 5])
@pytest.mark.parametrize("F", [4, 260, 1028])
def test_fp32_concap_finishing_equals_the_host_oracle(F, R, objective):
    """F = 4: one column group; 260: one partial block of 256 threads; 1028: a second block that holds a single group.
    R = 3: fewer rows than the loop's unroll of 4; 5: one unrolled pass and a remainder."""
    from vilbert import input_pipeline as ip
    raw, want = _concap_oracle(F, R, False)
    _equals_oracle(ip.finish_batch(_to_dev(raw), objective), want[objective])


@pytest.mark.parametrize("objective", [0, 1])
@pytest.mark.parametrize("R", [5, 9])
@pytest.mark.parametrize("F", [8, 264])
def test_float16_concap_finishing_equals_the_host_oracle_on_the_widened_features(F, R, objective):
    """R = 9 crosses the 8 rows in flight by one; both output kinds."""
    from vilbert import input_pipeline as ip
    raw, want = _concap_oracle(F, R, True)
    dev = _to_dev(raw)
    _equals_oracle(ip.finish_batch(dev, objective), want[objective])
    _equals_oracle(ip.finish_batch(dev, objective, out_dtype=torch.bfloat16), want[objective], bf16=True)


def test_float16_concap_finishing_with_row_flags_equals_the_host_oracle_on_the_cleared_features():
    from vilbert import input_pipeline as ip
    c = wc.MASK_CASE
    raw, feat = wc.mask_case_raw()
    masked = mr.mask_batch(raw, c["seed"], wc.VOCAB, wc.MASK_ID, c["p"])        # host: the flagged fp32 rows are zeros
    want = bo.finish_batch(masked, 0)
    dev = _to_dev(dict(masked, image_feat=feat, zero_row=wc.mask_case_flags(raw)))
    _equals_oracle(ip.finish_batch(dev, 0), want)
    _equals_oracle(ip.finish_batch(dev, 0, out_dtype=torch.bfloat16), want, bf16=True)


@pytest.mark.parametrize("F", [8, 264])
def test_float16_task_builder_equals_the_host_restatement_on_the_widened_rows(F):
    """max_regions = 6; samples of 0, 1, 5, 9 and 12 rows: empty, a mean only, a fit, more than the 8 rows in flight, one
    that is truncated; the sample of 5 rows takes its mean over 3. Both output kinds."""
    from vilbert import task_pipeline as tp
    packed = tr.make_packed([0, 1, 5, 9, 12], F, seed=F, mean_rows=[0, 1, 3, 9, 12])
    half, wide = _narrow_packed(packed, F + 1)
    want = tr.finish_task_batch(wide, 6)
    assert want[2].sum(1).tolist() == [1, 2, 6, 6, 6] and not want[0][0].any()
    dev = _to_dev(half)
    for out_dtype in (torch.float32, torch.bfloat16):
        got = tp.finish_task_batch(dev, 6, out_dtype=out_dtype)
        assert len(got) == 3
        _same(got[0].cpu(), torch.from_numpy(want[0]).to(out_dtype), "features, %s" % out_dtype)
        _same(got[1].cpu(), torch.from_numpy(want[1]), "spatials")
        _same(got[2].cpu(), torch.from_numpy(want[2]), "image_mask")


# ---- 5: the flat widening ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2051, 3 * 5 * 1601])
def test_widen_equals_numpys_cast_and_writes_nothing_behind_the_end(n):
    from vilbert import _native as N
    from vilbert import input_pipeline as ip
    x = wc.f16_values((n,), n)
    extra = np.array([0x7C00, 0xFC00, 0x7E00, 0xFE01, 0x7C01], dtype=np.uint16).view(np.float16)     # +-Inf, NaNs
    k = min(len(extra), n)
    x[n - k:] = extra[:k]                                   # (over the special finite values where n is that small)
    want = x.astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    guard = 16
    y = torch.full((n + guard,), -123.25, dtype=torch.float32, device=DEV)
    assert N.lib().vbw_widen_f16(N.stream_ptr(), n, xd.data_ptr(), y.data_ptr()) == 0
    torch.cuda.synchronize()
    host = y.cpu().numpy()
    assert (host[n:] == np.float32(-123.25)).all(), "the guard region was written"
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(host[:n]), nan)
    assert np.array_equal(host[:n][~nan].view(np.int32), want[~nan].view(np.int32))                  # signed zeros, subnormals
    assert nan.any() == (n >= 3) and np.isinf(want).any()
    api = ip.widen_f16(xd.view(1, n))
    assert api.shape == (1, n) and api.dtype == torch.float32
    assert np.array_equal(api.cpu().numpy().ravel()[~nan].view(np.int32), want[~nan].view(np.int32))


# ---- 6: the pipelines ----------------------------------------------------------------------------------------------------------
def _run(pipe):
    out = []
    for batch in pipe:
        out.append([t.clone() if isinstance(t, torch.Tensor) else t for t in batch])    # read before the slot is reused
        torch.cuda.current_stream().synchronize()
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["source-masked", "device-masked"])
def test_pretraining_pipeline_with_a_float16_wire_equals_the_default_on_the_widened_arrays(masked):
    from vilbert import input_pipeline as ip
    if masked:
        raws = [mr.make_unmasked_batch(4, tokens=10, regions=6, feat_dim=64, n_classes=9, vocab=99, seed=60 + i) for i in range(4)]
        fields = mr.RAW_UNMASKED_FIELDS
    else:
        raws = [bo.make_raw_batch(4, tokens=10, regions=6, feat_dim=64, n_classes=9, vocab=99, seed=50 + i) for i in range(4)]
        fields = bo.RAW_FIELDS
    for i, r in enumerate(raws):                        # 1601-like targets that are float16 values, full-mantissa features
        r["image_feat"] = wc.f16_values(r["image_feat"].shape, 70 + i)
        r["image_target"] = r["image_target"].astype(np.float16)
    half = [tuple(r[n] for n in fields) + ("id%d" % i,) for i, r in enumerate(raws)]
    wide = [tuple(wc.widen(r[n]) if n in ip.WIRE_FIELDS else r[n] for n in fields) + ("id%d" % i,) for i, r in enumerate(raws)]

    def masking():
        return ip.Masking(seed=77, vocab_size=99, mask_token_id=3, p_select=0.4) if masked else None

    want = _run(ip.DeviceBatchPipeline(wide, DEV, objective=1, masking=masking()))
    pipe = ip.DeviceBatchPipeline(half, DEV, objective=1, masking=masking(), wire_dtype=torch.float16)
    got = _run(pipe)
    got16 = _run(ip.DeviceBatchPipeline(half, DEV, objective=1, masking=masking(), wire_dtype=torch.float16,
                                        feature_dtype=torch.bfloat16))
    assert len(got) == len(got16) == len(want) == 4                            # two slots, each used twice
    assert pipe.slots[0].dev["image_feat"].dtype == torch.float16 and pipe.slots[0].dev["image_target"].dtype == torch.float16
    for i in range(4):
        assert len(got[i]) == 11 and got[i][10] == got16[i][10] == "id%d" % i
        for j in range(10):
            _same(got[i][j], want[i][j], "batch %d item %d" % (i, j))
            _same(got16[i][j].cpu(), _round_bf16(want[i][j]) if j == 5 else want[i][j].cpu(), "bf16 batch %d item %d" % (i, j))
        assert got[i][7].dtype == torch.float32 and got16[i][5].dtype == torch.bfloat16
    if masked:
        assert any((w[8] == 1).any() for w in want)                             # regions were selected


@pytest.mark.parametrize("target", [("dense", 11), ("iou", 0.5)], ids=["dense", "iou"])
def test_task_pipeline_with_a_float16_wire_equals_the_default_on_the_widened_arrays(target):
    from vilbert import task_pipeline as tp
    from test_task_batch_gpu import _task_batches
    R, T = 6, 9
    wide = _task_batches(16, R, T, 11, seed=40) + _task_batches(16, R, T, 11, seed=90)[:1]
    half = []
    for i, b in enumerate(wide):
        h = wc.f16_values(b["feat"].shape, 30 + i)
        half.append(dict(b, feat=h))
        b["feat"] = wc.widen(h)
    want = _run(tp.TaskBatchPipeline(wide, DEV, R, target=target))
    pipe = tp.TaskBatchPipeline(half, DEV, R, target=target, wire_dtype=torch.float16)
    got = _run(pipe)
    got16 = _run(tp.TaskBatchPipeline(half, DEV, R, target=target, wire_dtype=torch.float16, feature_dtype=torch.bfloat16))
    assert len(got) == len(got16) == len(want) == 4 and pipe.slots[0].dev["feat"].dtype == torch.float16
    for i in range(4):
        assert len(got[i]) == 9
        for j in range(9):
            _same(got[i][j], want[i][j], "batch %d item %d" % (i, j))
            _same(got16[i][j].cpu(), _round_bf16(want[i][j]) if j == 0 else want[i][j].cpu(), "bf16 batch %d item %d" % (i, j))
        assert got16[i][0].dtype == torch.bfloat16


# ---- 7: the model takes the bf16 block as it is ----------------------------------------------------------------------------------
NAMES = ["input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "masked_lm_labels", "image_label", "image_target", "next_sentence_label"]


@pytest.fixture
def det():
    from vilbert import _native
    wanted = _native._DET["wanted"]
    _native.set_deterministic(True)
    yield _native
    _native.set_deterministic(wanted)


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16-stream", "fp32-stream"])
def test_model_gives_the_same_bits_from_a_bf16_feature_block_as_from_its_widening(det, bf16):
    from vilbert import ops16
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    cfg = synth.load_config("bert_base_2layer_2conect.json")
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
    model.load_state_dict(synth.make_state_dict(cfg, "pretraining"))
    model = model.to(DEV).eval()                                               # dropout off, autograd on
    if bf16:
        model.half()
    x = synth.make_inputs(cfg, 2, 8, 5, seed=3, with_labels=True)
    feat16 = x["image_feat"].to(torch.bfloat16).to(DEV)
    args = [x[n].to(DEV) for n in NAMES]
    weight = model.bert.v_embeddings.image_embeddings.weight
    casts = []
    orig = ops16.cast_bf16
    ops16.cast_bf16 = lambda t: (casts.append(tuple(t.shape)), orig(t))[1]
    try:
        runs = []
        for feat in (feat16, feat16.float()):
            model.zero_grad(set_to_none=True)
            del casts[:]
            args[1] = feat
            loss = sum(l.mean() for l in model(*args))
            loss.backward()
            torch.cuda.synchronize()
            runs.append((loss.detach().clone(), weight.grad.clone(), [s for s in casts if s[-1] == feat.shape[-1]]))
    finally:
        ops16.cast_bf16 = orig
    assert torch.isfinite(runs[0][0]) and runs[0][1].abs().max() > 0
    assert torch.equal(runs[0][0], runs[1][0]), (runs[0][0].item(), runs[1][0].item())
    assert torch.equal(runs[0][1], runs[1][1])
    if bf16:
        assert runs[0][2] == [] and len(runs[1][2]) == 1                       # no cast launch for the bf16 block
