"""Cost of building one fine-tuning batch at the VQA shape (128 samples, 101 regions, 2048 features, 10 .. 100 detector boxes per
image, 10 sparse answers, 3,129 labels):

  host, reference-shaped   per sample the work the reference's datasets do in numpy (mean-region row, 5-number boxes, float64 zero
                           padding to 101 regions, back to float32, dense answer target), then the stack of the samples, then
                           the host-to-device copy of the padded tensors. Wall clock up to a device synchronise.
                             1 core       one process
                             N workers    the per-sample part spread over N forked worker processes (started before the GPU is
                                          touched; each returns its stacked share), stack and copy in the parent
  packed                   vilbert.task_pipeline: host concatenation of the packed arrays (pack_task_samples), their copy, then
                           vbd_task_finish_batch + vbd_dense_target. Wall clock up to a device synchronise.
  kernels                  device events around back-to-back launches through the C ABI into preallocated outputs:
                             task inputs  vbd_task_finish_batch (the feature kernel plus the small box / mask kernel); the GB/s
                                          figure charges ALL of that time to the feature kernel's 4 F (N + B R) bytes
                             concap       vb_concap_finish_batch (csrc/batch.hip: concap_feat_kernel<float, float> of
                                          csrc/feat_rows.h plus its label kernel) at an equal byte count: the yardstick
                                          already in the tree
                             dense target vbd_dense_target
                           Both feature kernels rotate through four sets of feature buffers (660 MB, beyond the 256 MiB
                           last-level cache), so their GB/s are figures for memory traffic, not for cache hits.

Every leg is warmed up, then timed REPEATS times with the two kernels alternating; median and the range of the repeats are printed.
The outputs of the host and device legs are compared bit for bit before anything is timed. Needs a GPU.

    python tools/task_batch_bench.py [--iters 200] [--warmup 20] [--host-iters 5] [--workers 16]
"""
import argparse
import ctypes
import multiprocessing
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import task_batch_restatement as tr  # noqa: E402

DEV = "cuda:0"
B, R, F, K, LABELS = 128, 101, 2048, 10, 3129
REPEATS = 5
SETS = 4          # feature buffer sets the kernel legs rotate through


def make_samples(seed=1):
    rng = np.random.default_rng(seed)
    n_rows = rng.integers(10, 101, B).tolist()
    packed = tr.make_packed(n_rows, F, seed=seed)
    off = packed["offsets"]
    samples = [dict(feat=packed["feat"][off[b]:off[b + 1]].copy(), boxes=packed["boxes"][off[b]:off[b + 1]].copy(),
                    image_w=int(packed["image_wh"][b, 0]), image_h=int(packed["image_wh"][b, 1])) for b in range(B)]
    labels = np.stack([rng.permutation(LABELS)[:K] for _ in range(B)]).astype(np.int32)
    labels[:, 3:][rng.uniform(size=(B, K - 3)) < 0.5] = -1
    scores = rng.choice(np.array([0.3, 0.6, 0.9, 1.0], dtype=np.float32), (B, K))
    return samples, labels, scores


def host_sample(s, labels, scores):
    """One padded sample built on the host with the work the reference's datasets spend on it - an fp32 mean row, the box
    arithmetic, a float64 [R, F] pad and its conversion back to fp32, the region mask and a dense answer target - laid out as
    tests/task_batch_restatement.py lays it out (straight into the padded rows). The bits are the device's (checked in main)."""
    feat, boxes = s["feat"], s["boxes"]
    kept = min(feat.shape[0] + 1, R)
    w, h, area = np.float32(s["image_w"]), np.float32(s["image_h"]), np.float32(s["image_w"] * s["image_h"])
    feat_pad = np.zeros((R, F), dtype=np.float64)
    feat_pad[0] = feat.sum(axis=0, dtype=np.float32) / np.float32(feat.shape[0])
    feat_pad[1:kept] = feat[:kept - 1]
    px = boxes[:kept - 1]
    spat_pad = np.zeros((R, 5), dtype=np.float64)
    spat_pad[0, 2:] = 1
    spat_pad[1:kept, 0:4:2] = px[:, 0:4:2] / w
    spat_pad[1:kept, 1:4:2] = px[:, 1:4:2] / h
    spat_pad[1:kept, 4] = ((px[:, 3] - px[:, 1]) * (px[:, 2] - px[:, 0])) / area
    target = np.zeros(LABELS, dtype=np.float32)
    real = labels >= 0
    target[labels[real]] = scores[real]
    return feat_pad.astype(np.float32), spat_pad.astype(np.float32), (np.arange(R) < kept).astype(np.int64), target


def host_share(job):
    samples, labels, scores = job
    items = [host_sample(s, labels[i], scores[i]) for i, s in enumerate(samples)]
    return [np.stack(col) for col in zip(*items)]


def host_batch(samples, labels, scores, pool=None, workers=0):
    t0 = time.perf_counter()
    if pool is None:
        items = [host_sample(s, labels[i], scores[i]) for i, s in enumerate(samples)]
        cols = [torch.from_numpy(np.stack(col)) for col in zip(*items)]
    else:
        cuts = np.linspace(0, B, workers + 1).astype(int)
        shares = pool.map(host_share, [(samples[a:b], labels[a:b], scores[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
        cols = [torch.from_numpy(np.concatenate(col)) for col in zip(*shares)]
    out = [c.to(DEV, non_blocking=True) for c in cols]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def packed_batch(samples, labels, scores):
    from vilbert import task_pipeline as tp
    t0 = time.perf_counter()
    packed = tp.pack_task_samples(samples)
    dev = {k: torch.from_numpy(v).to(DEV, non_blocking=True) for k, v in packed.items()}
    lab, sc = torch.from_numpy(labels).to(DEV, non_blocking=True), torch.from_numpy(scores).to(DEV, non_blocking=True)
    out = tp.finish_task_batch(dev, R) + (tp.dense_target(lab, sc, LABELS),)
    torch.cuda.synchronize()
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


def kernel_launchers(samples, labels, scores):
    """Closures that launch through the C ABI into preallocated buffers (a ctypes call per launch pair, nothing else). The two
    feature kernels rotate through SETS copies of their feature input and output - SETS x 165 MB, more than the 256 MiB last-level
    cache holds - so a launch finds neither its input nor its output lines left over from the launch before."""
    from vilbert import _native as N
    from vilbert import task_pipeline as tp
    lib = N.lib()
    packed = {k: torch.from_numpy(v).to(DEV) for k, v in tp.pack_task_samples(samples).items()}
    n = packed["feat"].shape[0]
    keep = [packed, torch.empty(B, R, 5, device=DEV), torch.empty(B, R, dtype=torch.int64, device=DEV)]
    task_args = []
    for _ in range(SETS):
        a = N.TaskBatchArgs()
        a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.total_rows = B, R, F, 0.0, n
        feat_in, feat_out = packed["feat"].clone(), torch.empty(B, R, F, device=DEV)
        a.feat, a.out_feat = feat_in.data_ptr(), feat_out.data_ptr()
        a.boxes, a.offsets, a.image_wh, a.mean_rows = (packed[k].data_ptr() for k in tp.PACKED_FIELDS[1:])
        a.out_spatials, a.out_mask = keep[1].data_ptr(), keep[2].data_ptr()
        task_args.append(a)
        keep += [feat_in, feat_out]
    task_bytes = 4 * F * (n + B * R)

    # the pre-training finisher at an equal byte count: 4 F B (2 Rc + 1) bytes
    Rc, T = max(1, round((task_bytes / (4 * F * B) - 1) / 2)), 36
    small = dict(image_loc=torch.rand(B, Rc, 5, device=DEV), image_mask=torch.ones(B, Rc, dtype=torch.int64, device=DEV),
                 masked_label=torch.zeros(B, Rc, dtype=torch.int64, device=DEV), is_next=torch.zeros(B, dtype=torch.int64, device=DEV),
                 image_label=torch.zeros(B, Rc, dtype=torch.int64, device=DEV),
                 lm_label_ids=torch.zeros(B, T, dtype=torch.int64, device=DEV),
                 out_image_loc=torch.empty(B, Rc + 1, 5, device=DEV), out_image_mask=torch.empty(B, Rc + 1, dtype=torch.int64, device=DEV),
                 out_image_label=torch.empty(B, Rc, dtype=torch.int64, device=DEV),
                 out_lm_label_ids=torch.empty(B, T, dtype=torch.int64, device=DEV))
    concap_args = []
    for _ in range(SETS):
        c = N.ConcapBatch()
        c.batch, c.regions, c.tokens, c.feat_dim, c.objective = B, Rc, T, F, 0
        big = dict(image_feat=torch.randn(B, Rc, F, device=DEV), out_image_feat=torch.empty(B, Rc + 1, F, device=DEV))
        for k, t in list(small.items()) + list(big.items()):
            setattr(c, k, t.data_ptr())
        concap_args.append(c)
        keep.append(big)
    concap_bytes = 4 * F * B * (2 * Rc + 1)

    lab, sc = torch.from_numpy(labels).to(DEV), torch.from_numpy(scores).to(DEV)
    tgt = torch.empty(B, LABELS, device=DEV)
    keep += [small, lab, sc, tgt]
    turn = {"task": 0, "concap": 0}

    def task():
        turn["task"] = (turn["task"] + 1) % SETS
        N.check(lib.vbd_task_finish_batch(N.stream_ptr(), ctypes.byref(task_args[turn["task"]])), "vbd_task_finish_batch")

    def concap():
        turn["concap"] = (turn["concap"] + 1) % SETS
        N.check(lib.vb_concap_finish_batch(N.stream_ptr(), ctypes.byref(concap_args[turn["concap"]])), "vb_concap_finish_batch")

    def dense():
        N.check(lib.vbd_dense_target(N.stream_ptr(), B, LABELS, K, lab.data_ptr(), sc.data_ptr(), tgt.data_ptr(), LABELS),
                "vbd_dense_target")

    return dict(task=(task, task_bytes), concap=(concap, concap_bytes), dense=(dense, 4 * B * LABELS)), keep, n, Rc


def show(name, values, unit="ms per batch"):
    print("  %-28s median %9.4f %s   (range %.4f .. %.4f over %d repeats)"
          % (name, statistics.median(values), unit, min(values), max(values), len(values)))
    return statistics.median(values)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    ap.add_argument("--workers", type=int, default=16, help="0: skip the multi-worker host leg")
    args = ap.parse_args()
    samples, labels, scores = make_samples()
    # the workers are forked BEFORE this process touches the GPU; they only ever run numpy / CPU torch
    pool = multiprocessing.get_context("fork").Pool(args.workers, torch.set_num_threads, (1,)) if args.workers > 0 else None
    try:
        if not torch.cuda.is_available():
            raise SystemExit("task_batch_bench needs a GPU - nothing is measured without one")
        _, host_out = host_batch(samples, labels, scores)
        _, dev_out = packed_batch(samples, labels, scores)
        for h, d in zip(host_out, dev_out):
            assert h.dtype == d.dtype and torch.equal(h, d)
        if pool is not None:
            for h, d in zip(host_batch(samples, labels, scores, pool, args.workers)[1], dev_out):
                assert torch.equal(h, d)
        launch, keep, n, Rc = kernel_launchers(samples, labels, scores)
        padded_mb = sum(t.numel() * t.element_size() for t in host_out) / 1e6
        packed_mb = (n * (F + 4) * 4 + B * (8 + 8 + 4) + B * K * 8) / 1e6
        print("one VQA-shaped batch: %d samples, %d regions, %d features, %d packed rows (%.1f per sample), %d answers, %d labels; "
              "host-built and device-built tensors agree bit for bit" % (B, R, F, n, n / B, K, LABELS))
        print("  copied host to device: padded %.1f MB, packed %.1f MB" % (padded_mb, packed_mb))
        res = {"host 1 core": [], "host %d workers" % args.workers: [], "packed": [], "task": [], "concap": [], "dense": []}
        for fn, _ in launch.values():
            event_leg(fn, args.warmup, args.warmup)
        for _ in range(REPEATS):
            res["host 1 core"].append(statistics.median(host_batch(samples, labels, scores)[0] for _ in range(args.host_iters)))
            if pool is not None:
                res["host %d workers" % args.workers].append(statistics.median(
                    host_batch(samples, labels, scores, pool, args.workers)[0] for _ in range(args.host_iters)))
            res["packed"].append(statistics.median(packed_batch(samples, labels, scores)[0] for _ in range(args.host_iters)))
            for name in ("task", "concap", "dense"):
                res[name].append(event_leg(launch[name][0], args.warmup, args.iters))
        host1 = show("host, 1 core", res["host 1 core"])
        hostn = show("host, %d workers" % args.workers, res["host %d workers" % args.workers]) if pool is not None else None
        packed = show("packed (pack, copy, launch)", res["packed"])
        print("  host 1 core / packed = %.1fx" % (host1 / packed) + ("" if hostn is None else
                                                                  "   host %d workers / packed = %.1fx" % (args.workers, hostn / packed)))
        for name, label in (("task", "kernels: task inputs"), ("concap", "kernels: concap (R = %d)" % Rc), ("dense", "kernels: dense target")):
            med = show(label, res[name])
            print("      %.1f MB -> %.0f GB/s" % (launch[name][1] / 1e6, launch[name][1] / 1e6 / med))
    finally:
        if pool is not None:
            pool.terminate()
            pool.join()


if __name__ == "__main__":
    main()
