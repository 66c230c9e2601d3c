"""Generates tests/golden/task_batch.npz: a handful of detector records and what the REFERENCE's own fine-tuning datasets make
of them - ImageFeaturesH5Reader.__getitem__, VQAClassificationDataset.__getitem__ and ReferExpressionDataset.__getitem__ (train
and val split), imported from the reference checkout and run as they are. Inputs and outputs only are stored.

The three modules are loaded one by one under an alias package (so the reference's datasets/__init__.py, which pulls in every
loader, does not run), with `lmdb`, `h5py`, `tools.refer.refer` and the tokenizer module stubbed in sys.modules (none of them
is reached by __getitem__). The objects are made with object.__new__ and given the handful of attributes __getitem__ reads; the
reader's `env` is a fake whose transaction returns pickled records.

The feature values are multiples of 1/16 below 16 (half of them zero, like post-ReLU detector features), so the file compresses;
their sums are exact, which is why the order of the column sum is pinned by tests/test_task_batch.py on full-mantissa data and
not by this file. Run in the build container:  python tests/golden/make_task_batch_golden.py"""
import importlib
import os
import pickle
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader  # noqa: E402

ALIAS = "vilbert_reference_datasets"
MAX_REGIONS, SEQ, NUM_LABELS, K = 6, 8, 23, 4
# image id -> (regions, width, height): with max_region_num = 6 the n + 1 rows of a sample lie below, at and above it;
# 5000 x 4000 exceeds 2^24
IMAGES = {11: (3, 640, 480), 12: (5, 5000, 4000), 13: (6, 500, 375), 14: (9, 333, 500)}
GT_IMAGES = {11: 2, 13: 1}              # ground-truth boxes the refer-expression training split appends


def load_reference_datasets():
    saved = {n: sys.modules.get(n) for n in ("lmdb", "h5py", "tools", "tools.refer", "tools.refer.refer", "pytorch_transformers",
                                            "pytorch_transformers.tokenization_bert")}
    for name in saved:
        sys.modules[name] = types.ModuleType(name)
    sys.modules["tools.refer.refer"].REFER = object
    sys.modules["pytorch_transformers.tokenization_bert"].BertTokenizer = object      # (an annotation of the constructor)
    pkg = types.ModuleType(ALIAS)
    pkg.__path__ = [os.path.join(ref_loader.REFERENCE_ROOT, "vilbert", "datasets")]
    sys.modules[ALIAS] = pkg
    try:
        return [importlib.import_module(ALIAS + "." + n)
                for n in ("_image_features_reader", "vqa_dataset", "refer_expression_dataset")]
    finally:
        for name, mod in saved.items():
            if mod is None:
                del sys.modules[name]
            else:
                sys.modules[name] = mod


class FakeEnv(object):
    """lmdb environment of pickled records: env.begin(write=False) is a context manager with get(key)."""

    def __init__(self, records):
        self.records = {str(k).encode(): pickle.dumps(v) for k, v in records.items()}

    def begin(self, write=False):
        return self

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False

    def get(self, key):
        return self.records[key]


def make_records(rng, sizes):
    records = {}
    for image_id, (n, w, h) in sizes.items():
        feat = rng.integers(0, 256, (n, 2048)) * rng.integers(0, 2, (n, 2048)) / 16.0
        lo = rng.uniform(0, 0.6, (n, 2)) * (w, h)
        hi = lo + rng.uniform(0.05, 0.4, (n, 2)) * (w, h)
        boxes = np.concatenate([lo, hi], axis=1).astype(np.float32)
        # the LMDB record of the feature extractor: flat arrays, sizes as numbers
        records[image_id] = dict(image_id=image_id, image_h=h, image_w=w, num_boxes=n,
                                 features=feat.astype(np.float32).reshape(-1), boxes=boxes.reshape(-1))
    return records


def make_reader(mod, records):
    reader = object.__new__(mod.ImageFeaturesH5Reader)
    reader.env, reader._in_memory = FakeEnv(records), False
    reader._image_ids = [str(k).encode() for k in records]
    return reader


def tokens(rng):
    n = int(rng.integers(3, SEQ + 1))
    ids = np.zeros(SEQ, dtype=np.int64)
    ids[:n] = rng.integers(1000, 2000, n)
    mask = (np.arange(SEQ) < n).astype(np.int64)
    return torch.from_numpy(ids), torch.from_numpy(mask), torch.zeros(SEQ, dtype=torch.int64)


def stack(items, idx):
    return np.stack([np.asarray(it[idx]) for it in items])


def main():
    rng = np.random.default_rng(20)
    reader_mod, vqa_mod, refer_mod = load_reference_datasets()
    records = make_records(rng, IMAGES)
    gt_records = make_records(rng, {i: (g,) + IMAGES[i][1:] for i, g in GT_IMAGES.items()})
    reader, gt_reader = make_reader(reader_mod, records), make_reader(reader_mod, gt_records)

    save = dict(max_regions=MAX_REGIONS, num_labels=NUM_LABELS)
    for tag, recs in (("img", records), ("gt", gt_records)):
        save[tag + "_ids"] = np.array(list(recs), dtype=np.int64)
        save[tag + "_rows"] = np.array([r["num_boxes"] for r in recs.values()], dtype=np.int64)
        save[tag + "_wh"] = np.array([(r["image_w"], r["image_h"]) for r in recs.values()], dtype=np.int32)
        save[tag + "_feat"] = np.concatenate([r["features"].reshape(-1, 2048) for r in recs.values()])
        save[tag + "_boxes"] = np.concatenate([r["boxes"].reshape(-1, 4) for r in recs.values()])

    # the reader alone, first image: (features, num_boxes, boxes, boxes_ori)
    f, n, loc, loc_ori = reader[11]
    save.update(reader_features=f, reader_num_boxes=n, reader_boxes=loc, reader_boxes_ori=loc_ori)

    # VQA: sparse answers (one sample without any), dense [num_labels] target
    vqa = object.__new__(vqa_mod.VQAClassificationDataset)
    vqa._image_features_reader, vqa._max_region_num, vqa._max_seq_length = reader, MAX_REGIONS, SEQ
    vqa.num_labels, vqa.split, vqa.entries = NUM_LABELS, "train", []
    labels = np.full((len(IMAGES), K), -1, dtype=np.int32)
    scores = np.zeros((len(IMAGES), K), dtype=np.float32)
    for e, image_id in enumerate(IMAGES):
        k = (3, 0, 1, 4)[e]
        labels[e, :k] = rng.permutation(NUM_LABELS)[:k]
        if e == 0:
            labels[e, :2] = (0, NUM_LABELS - 1)
        scores[e, :k] = rng.choice(np.array([0.3, 0.6, 0.9, 1.0], dtype=np.float32), k)
        q, m, s = tokens(rng)
        answer = dict(labels=torch.from_numpy(labels[e, :k].astype(np.int64)) if k else None,
                      scores=torch.from_numpy(scores[e, :k].copy()) if k else None)
        vqa.entries.append(dict(image_id=image_id, question_id=100 + e, q_token=q, q_input_mask=m, q_segment_ids=s,
                                answer=answer))
    items = [vqa[i] for i in range(len(vqa.entries))]
    save.update(vqa_image=np.array(list(IMAGES), dtype=np.int64), vqa_labels=labels, vqa_scores=scores,
                vqa_features=stack(items, 0), vqa_spatials=stack(items, 1), vqa_image_mask=stack(items, 2),
                vqa_question=stack(items, 3), vqa_target=stack(items, 4), vqa_input_mask=stack(items, 5),
                vqa_segment_ids=stack(items, 6), vqa_co_attention_mask=stack(items, 7),
                vqa_question_id=np.array([it[8] for it in items], dtype=np.int64))

    # refer expressions: refBox is x, y, width, height. val: IoU of every row, no floor; train: the ground-truth rows are
    # appended and IoU below 0.5 becomes 0 (the reference box of image 11 IS its first ground-truth box: IoU 1)
    def gt_xywh(image_id, j):
        x1, y1, x2, y2 = (float(v) for v in gt_records[image_id]["boxes"].reshape(-1, 4)[j])
        return [x1, y1, x2 - x1, y2 - y1]

    def det_xywh(image_id, j, grow):
        x1, y1, x2, y2 = (float(v) for v in records[image_id]["boxes"].reshape(-1, 4)[j])
        return [x1, y1, (x2 - x1) * grow, (y2 - y1) * grow]

    for split, entries in (("val", [(11, det_xywh(11, 1, 1.25)), (12, det_xywh(12, 0, 0.8)), (14, det_xywh(14, 3, 1.0))]),
                           ("train", [(11, gt_xywh(11, 0)), (13, det_xywh(13, 2, 1.5))])):
        ds = object.__new__(refer_mod.ReferExpressionDataset)
        ds._image_features_reader, ds._gt_image_features_reader = reader, gt_reader
        ds.split, ds.max_region_num, ds._max_seq_length, ds.entries = split, MAX_REGIONS, SEQ, []
        for image_id, box in entries:
            t, m, s = tokens(rng)
            ds.entries.append(dict(image_id=image_id, refBox=box, token=t, input_mask=m, segment_ids=s))
        items = [ds[i] for i in range(len(ds.entries))]
        p = "refer_%s_" % split
        save.update({p + "image": np.array([e[0] for e in entries], dtype=np.int64),
                     p + "ref_xywh": np.array([e[1] for e in entries], dtype=np.float64),
                     p + "features": stack(items, 0), p + "spatials": stack(items, 1), p + "image_mask": stack(items, 2),
                     p + "target": stack(items, 4)})
    path = os.path.join(HERE, "task_batch.npz")
    np.savez_compressed(path, **save)
    print("wrote task_batch.npz (%d bytes)" % os.path.getsize(path), {k: np.shape(v) for k, v in save.items()})


if __name__ == "__main__":
    main()
