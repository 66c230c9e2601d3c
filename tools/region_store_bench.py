"""Cost of one fine-tuning batch from the device-resident region store (vilbert.region_store) against the packed path
(vilbert.task_pipeline), at the VQA shape: 128 samples, 101 regions, 2048 columns, 10 .. 100 detector boxes per image, binary16
features, fp32 feature block, 10 sparse answers over 3,129 labels, 23 tokens. Method of tools/task_batch_bench.py.

  1 per batch     wall clock from the host's arrays to a device synchronise, through the pipelines:
                    packed   pack_task_samples (host concatenation) + TaskBatchPipeline: the copy of the packed arrays, then
                             vbw_task_finish_batch + vbd_dense_target
                    store    StoreBatchPipeline: the copy of 128 image ids (and the same token / answer arrays), then
                             vbr_store_finish_batch + vbd_dense_target
  2 kernels only  device events around back-to-back launches through the C ABI into preallocated outputs. The store holds at
                  least 1 GB (beyond the 256 MiB last-level cache) and a launch gathers 128 ids drawn at random from it; the packed
                  twin is vbw_task_finish_batch on the same images packed. Both rotate through the same ID_SETS draws and
                  OUT_SETS output blocks - more input and output bytes than the cache holds - and the two alternate. The
                  body of the two is the same kernel: the store may be behind by the packed kernel's own min .. max range over
                  the repeats plus 3 % (the gap between task_feat_kernel and concap_feat_kernel at equal bytes,
                  profiles/task_batch_ab.txt).
  3 repeated ids  leg 2 with 32 images shown 4 times each (the VCR shape) - for the record.

Every leg is warmed up, then timed REPEATS times; median and the range of the repeats are printed. The outputs of the two paths
are compared bit for bit before anything is timed. Needs a GPU. Prints, and writes the same lines to --out.

    python tools/region_store_bench.py [--iters 200] [--warmup 20] [--host-iters 5] [--out profiles/region_store_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
B, R, F, K, LABELS, T = 128, 101, 2048, 10, 3129, 23
REPEATS = 5
IMAGES, CHUNK = 5120, 512      # 5120 images of 10 .. 100 rows of 4 KB: about 1.15 GB
ID_SETS, OUT_SETS = 16, 4      # 16 draws x 29 MB of rows read, 4 x 106 MB of blocks written
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def make_image(rng, rows):
    """One raw sample with float16 features (post-ReLU-like: non-negative, many zeros) - what ``raw_item`` hands over when
    the feature file keeps float16."""
    feat = np.maximum(rng.standard_normal((rows, F), dtype=np.float32) - 0.5, 0).astype(np.float16)
    w, h = (int(v) for v in rng.integers(200, 1000, 2))
    lo = rng.uniform(0, 0.7, (rows, 2)) * (w, h)
    boxes = np.concatenate([lo, lo + rng.uniform(0.01, 0.3, (rows, 2)) * (w, h)], axis=1).astype(np.float32)
    return dict(feat=feat, boxes=boxes, image_w=w, image_h=h)


def build_store(rng):
    """The store, filled chunk by chunk through the public API; returns it with the row count of every image."""
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    n_rows = rng.integers(10, 101, IMAGES)
    store = rs.RegionStore(DEV, int(n_rows.sum()), IMAGES, feat_dim=F, dtype=torch.float16)
    t0 = time.perf_counter()
    for i in range(0, IMAGES, CHUNK):
        store.add(tp.pack_task_samples([make_image(rng, int(n)) for n in n_rows[i:i + CHUNK]], dtype=np.float16))
    torch.cuda.synchronize()
    return store, n_rows, time.perf_counter() - t0


def host_samples(store, ids):
    """The images `ids` of the store back on the host as raw samples (the packed path's input)."""
    off, wh = store.image_offsets.cpu().numpy(), store.image_wh.cpu().numpy()
    return [dict(feat=store.feat[off[i]:off[i + 1]].cpu().numpy(), boxes=store.boxes[off[i]:off[i + 1]].cpu().numpy(),
                 image_w=int(wh[i, 0]), image_h=int(wh[i, 1])) for i in ids]


def token_arrays(rng):
    lens = rng.integers(4, T + 1, B)
    mask = (np.arange(T)[None] < lens[:, None]).astype(np.int64)
    labels = np.stack([rng.permutation(LABELS)[:K] for _ in range(B)]).astype(np.int32)
    labels[:, 3:][rng.uniform(size=(B, K - 3)) < 0.5] = -1
    return dict(question=rng.integers(1, 30000, (B, T)) * mask, input_mask=mask, segment_ids=np.zeros((B, T), np.int64),
                question_id=np.arange(B, dtype=np.int64), labels=labels,
                scores=rng.choice(np.array([0.3, 0.6, 0.9, 1.0], dtype=np.float32), (B, K)))


def one_batch(pipe, batch):
    """`batch` through `pipe` (its slots keep their buffers from call to call) up to a device synchronise."""
    pipe.source = [batch]
    out = next(iter(pipe))
    torch.cuda.synchronize()
    return out


def packed_wall(pipe, samples, tokens):
    from vilbert import task_pipeline as tp
    t0 = time.perf_counter()
    out = one_batch(pipe, dict(tokens, **tp.pack_task_samples(samples, dtype=np.float16)))
    return (time.perf_counter() - t0) * 1e3, out


def store_wall(pipe, ids, tokens):
    t0 = time.perf_counter()
    out = one_batch(pipe, dict(tokens, image_ids=ids))
    return (time.perf_counter() - t0) * 1e3, out


def event_leg(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_launchers(store, n_rows, draws):
    """(store launcher, packed launcher, bytes moved per launch, buffers to keep alive) over `draws` (a list of id arrays):
    closures that launch through the C ABI into preallocated buffers - a ctypes call per launch pair, nothing else. Launch j of
    either takes draw j % len(draws) and output block j % OUT_SETS; the two produce the same bits (checked here)."""
    from vilbert import _native as N
    lib = N.lib()
    off = store.image_offsets.cpu().numpy()
    outs = [(torch.empty(B, R, F, device=DEV), torch.empty(B, R, 5, device=DEV), torch.empty(B, R, dtype=torch.int64, device=DEV))
            for _ in range(2 * OUT_SETS)]
    keep, store_args, packed_args, rows_read = [outs], [], [], 0
    for j, ids in enumerate(draws):
        rows = torch.from_numpy(np.concatenate([np.arange(off[i], off[i + 1]) for i in ids])).to(DEV)
        packed = dict(feat=store.feat[rows], boxes=store.boxes[rows], image_wh=store.image_wh[torch.from_numpy(ids).to(DEV)],
                      offsets=torch.from_numpy(np.concatenate([[0], np.cumsum(n_rows[ids])]).astype(np.int64)).to(DEV))
        ids_dev = torch.from_numpy(ids).to(DEV)
        keep += [packed, ids_dev]
        rows_read += int(rows.shape[0])
        for k in range(OUT_SETS):                       # every (draw, output block) pair its own argument struct
            s, p = N.StoreBatchArgs(), N.WireTaskBatch()
            for a in (s, p):
                a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.out_kind = B, R, F, 0.0, 0
            s.feat_kind, s.total_rows, s.num_images = 1, store.total_rows, store.num_images
            s.feat, s.boxes, s.image_offsets, s.image_wh = (t.data_ptr() for t in (store.feat, store.boxes, store.image_offsets, store.image_wh))
            s.image_ids = ids_dev.data_ptr()
            p.total_rows = int(rows.shape[0])
            p.feat, p.boxes, p.offsets, p.image_wh = (packed[n].data_ptr() for n in ("feat", "boxes", "offsets", "image_wh"))
            for a, o in ((s, outs[k]), (p, outs[OUT_SETS + k])):
                a.out_feat, a.out_spatials, a.out_mask = (t.data_ptr() for t in o)
            store_args.append(s)
            packed_args.append(p)
        N.check(lib.vbr_store_finish_batch(N.stream_ptr(), ctypes.byref(store_args[-OUT_SETS])), "vbr_store_finish_batch")
        N.check(lib.vbw_task_finish_batch(N.stream_ptr(), ctypes.byref(packed_args[-OUT_SETS])), "vbw_task_finish_batch")
        torch.cuda.synchronize()
        for a, b in zip(outs[0], outs[OUT_SETS]):
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    turn = {"store": 0, "packed": 0}

    def pick(name):
        j = turn[name] = turn[name] + 1
        return (j % len(draws)) * OUT_SETS + j % OUT_SETS

    def store_launch():
        N.check(lib.vbr_store_finish_batch(N.stream_ptr(), ctypes.byref(store_args[pick("store")])), "vbr_store_finish_batch")

    def packed_launch():
        N.check(lib.vbw_task_finish_batch(N.stream_ptr(), ctypes.byref(packed_args[pick("packed")])), "vbw_task_finish_batch")

    return store_launch, packed_launch, 2 * F * rows_read / len(draws) + 4 * F * B * R, keep


def show(name, values, unit="ms per batch"):
    say("  %-34s median %9.4f %s   (range %.4f .. %.4f over %d repeats)"
        % (name, statistics.median(values), unit, min(values), max(values), len(values)))
    return statistics.median(values)


def kernel_leg(title, store, n_rows, draws, args):
    store_launch, packed_launch, nbytes, keep = kernel_launchers(store, n_rows, draws)
    for fn in (store_launch, packed_launch):
        event_leg(fn, args.warmup, args.warmup)
    res = {"store": [], "packed": []}
    for _ in range(REPEATS):
        res["packed"].append(event_leg(packed_launch, args.warmup, args.iters))
        res["store"].append(event_leg(store_launch, args.warmup, args.iters))
    say(title)
    packed = show("packed  vbw_task_finish_batch", res["packed"], "ms per launch pair")
    stored = show("store   vbr_store_finish_batch", res["store"], "ms per launch pair")
    say("      %.1f MB per launch pair -> packed %.0f GB/s, store %.0f GB/s; store / packed = %.4f"
        % (nbytes / 1e6, nbytes / 1e6 / packed, nbytes / 1e6 / stored, stored / packed))
    del keep
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "region_store_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("region_store_bench needs a GPU - nothing is measured without one")
    from vilbert import region_store as rs
    from vilbert import task_pipeline as tp
    rng = np.random.default_rng(1)
    store, n_rows, fill_s = build_store(rng)
    say("region store: %d images, %d rows of %d binary16 columns, %.2f GB on the device (features %.2f GB), filled in %.1f s "
        "(host data generation included)" % (store.num_images, store.total_rows, F, store.nbytes / 1e9,
                                            store.total_rows * F * 2 / 1e9, fill_s))
    draws = [rng.choice(IMAGES, B, replace=False).astype(np.int64) for _ in range(ID_SETS)]
    tokens = token_arrays(rng)

    # ---- 1: per batch, wall clock ----
    ids = draws[0]
    samples = host_samples(store, ids)
    packed_pipe = tp.TaskBatchPipeline([], DEV, R, target=("dense", LABELS), wire_dtype=torch.float16)
    store_pipe = rs.StoreBatchPipeline([], store, R, target=("dense", LABELS))
    want, got = packed_wall(packed_pipe, samples, tokens)[1], store_wall(store_pipe, ids, tokens)[1]
    for w, g in zip(want, got):
        assert w.dtype == g.dtype and torch.equal(w.view(torch.int32) if w.dtype == torch.float32 else w,
                                                  g.view(torch.int32) if g.dtype == torch.float32 else g)
    n = int(n_rows[ids].sum())
    small = sum(v.nbytes for v in tokens.values())
    say("one VQA-shaped batch: %d samples, %d regions, %d columns, %d packed rows (%.1f per sample); the 9-tuples of the two "
        "pipelines agree bit for bit" % (B, R, F, n, n / B))
    say("  copied host to device per batch: packed %.2f MB, store %.4f MB (%d bytes of image ids + %d of tokens and answers)"
        % ((n * (2 * F + 16) + B * 20 + small) / 1e6, (B * 8 + small) / 1e6, B * 8, small))
    for _ in range(3):
        packed_wall(packed_pipe, samples, tokens), store_wall(store_pipe, ids, tokens)
    res = {"packed": [], "store": []}
    for _ in range(REPEATS):
        res["packed"].append(statistics.median(packed_wall(packed_pipe, samples, tokens)[0] for _ in range(args.host_iters)))
        res["store"].append(statistics.median(store_wall(store_pipe, ids, tokens)[0] for _ in range(args.host_iters)))
    say("1 per batch, wall clock to a synchronise (median of %d batches per repeat)" % args.host_iters)
    packed = show("packed  pack + copy + launches", res["packed"])
    stored = show("store   ids + launches", res["store"])
    say("      packed / store = %.1fx" % (packed / stored))

    # ---- 2: kernels only ----
    k = kernel_leg("2 kernels only, device events (%d draws of %d random ids, %d output blocks, the two alternating)"
                   % (ID_SETS, B, OUT_SETS), store, n_rows, draws, args)
    med_p, med_s = statistics.median(k["packed"]), statistics.median(k["store"])
    allowed = med_p + (max(k["packed"]) - min(k["packed"])) + 0.03 * med_p
    say("      allowed: packed median + its range + 3 %% = %.4f ms; store median %.4f ms: %s"
        % (allowed, med_s, "within" if med_s <= allowed else "BEHIND by %.4f ms" % (med_s - allowed)))

    # ---- 3: repeated ids ----
    repeated = [np.repeat(d[:B // 4], 4) for d in draws]
    kernel_leg("3 repeated ids: 32 images shown 4 times each (for the record)", store, n_rows, repeated, args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
