"""Cost of choosing the MLM and region masks of one pre-training batch (256 samples, 36 tokens, 36 regions, 2048 features):

  host loops       what a worker pays per batch for choosing on the host, one core, wall clock:
                     restatement   tests/masking_restatement.py mask_sample per sample + zeroing the selected feature rows
                                   (the library's hash, vectorised per sample; the per-site loops in Python)
                     random        the same per-site rule driven by Python's `random.random()` per site, the shape of the
                                   loops the reference's workers run (random_word / random_region)
  device           vilbert.input_pipeline.mask_batch: vbi_concap_mask_batch + vbi_zero_rows, two launches, HIP events
                     in place      the pipeline's form (selected feature rows cleared where they are)
                     copy          inplace=False (every feature row written to a new tensor: 75 MB read + 75 MB written)

The host legs run --host-iters times, the device legs --iters times after --warmup; every leg three times, median reported.
The outputs of the device and restatement legs are compared bit for bit before anything is timed. Needs a GPU.

    python tools/mask_batch_bench.py [--iters 200] [--warmup 20] [--host-iters 5]
"""
import argparse
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import masking_restatement as mr  # noqa: E402
from vilbert import input_pipeline as ip  # noqa: E402

DEV = "cuda:0"
B, T, R, F = 256, 36, 36, 2048
VOCAB, MASK_ID, P, SEED = 30522, 103, 0.15, 0xBE7C4
REPEATS = 3


def host_restatement(raw):
    feat = raw["image_feat"].copy()
    L = max(T, R)
    t0 = time.perf_counter()
    for b in range(B):
        out = mr.mask_sample(b, L, raw["input_ids"][b], raw["input_mask"][b], raw["image_mask"][b], raw["overlaps"][b], SEED,
                             VOCAB, MASK_ID, P)
        feat[b][out[4] != 0] = 0
    return (time.perf_counter() - t0) * 1e3


def host_random(raw):
    """The rule of include/vilbert_hip_inputs.h, one `random.random()` per site, lists in and out as in a worker. Written from
    the header's statement of the rule (select, 80 / 10 / 10, 90 / 10, OR of the overlap rows), not from the reference's text."""
    feat = raw["image_feat"].copy()
    t0 = time.perf_counter()
    for b in range(B):
        n_tok, n_box = int(raw["input_mask"][b].sum()), int(raw["image_mask"][b].sum())
        tokens = raw["input_ids"][b, 1:n_tok - 1].tolist()
        labels = []
        for i, tok in enumerate(tokens):
            u = random.random()
            if u < P:
                v = u / P
                if v < 0.8:
                    tokens[i] = MASK_ID
                elif v < 0.9:
                    tokens[i] = random.randrange(VOCAB)
                labels.append(tok)
            else:
                labels.append(-1)
        ov, region_labels, masked = raw["overlaps"][b], [], np.zeros(R, dtype=bool)
        for i in range(n_box):
            u = random.random()
            if u < P:
                if u / P < 0.9:
                    feat[b, i] = 0
                masked = np.logical_or(masked, ov[i] > 0.4)
                region_labels.append(1)
            else:
                region_labels.append(-1)
    return (time.perf_counter() - t0) * 1e3


def device_leg(dev, inplace, warmup, iters):
    fn = lambda: ip.mask_batch(dev, SEED, VOCAB, MASK_ID, P, inplace=inplace)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-iters", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mask_batch_bench needs a GPU - nothing is measured without one")
    raw = mr.make_unmasked_batch(B, tokens=T, regions=R, feat_dim=F, n_classes=2, vocab=VOCAB, seed=1)
    want = mr.mask_batch(raw, SEED, VOCAB, MASK_ID, P)
    to_dev = lambda: {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in raw.items()}
    for inplace in (False, True):
        got = ip.mask_batch(to_dev(), SEED, VOCAB, MASK_ID, P, inplace=inplace)
        for n in ip.RAW_FIELDS:
            assert np.array_equal(got[n].cpu().numpy(), want[n]), n
    print("masks of one batch: %d samples, %d tokens, %d regions, %d features, p_select %.2f (%d tokens, %d regions selected, "
          "%d feature rows cleared); device and restatement agree bit for bit"
          % (B, T, R, F, P, (want["lm_label_ids"] != -1).sum(), (want["image_label"] == 1).sum(),
             (want["image_feat"].reshape(B * R, F)[raw["image_mask"].reshape(-1) != 0] == 0).all(1).sum()))
    dev = to_dev()
    res = {"host restatement": [], "host random": [], "device in place": [], "device copy": []}
    for _ in range(REPEATS):
        res["host restatement"].append(statistics.median(host_restatement(raw) for _ in range(args.host_iters)))
        res["host random"].append(statistics.median(host_random(raw) for _ in range(args.host_iters)))
        res["device in place"].append(device_leg(dev, True, args.warmup, args.iters))
        res["device copy"].append(device_leg(dev, False, args.warmup, args.iters))
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print("  %-18s median %9.4f ms per batch   (%s)" % (k, med[k], "  ".join("%.4f" % x for x in v)))
    for h in ("host restatement", "host random"):
        print("  %s / device in place = %.0fx   (%.1f us per sample on one host core)"
              % (h, med[h] / med["device in place"], med[h] * 1e3 / B))
    print("  device copy moves %.0f MB: %.0f GB/s" % (2 * B * R * F * 4 / 1e6, 2 * B * R * F * 4 / 1e6 / med["device copy"]))


if __name__ == "__main__":
    main()
