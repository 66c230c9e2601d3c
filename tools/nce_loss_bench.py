"""Cost of the NCE masked-region loss (visual_target == 2, reference vilbert.py:1523-1575) alone, forward + backward, at the
pre-training shape: 256 samples x 36 regions, 2048-wide features, ~15 % of the regions labelled, num_negative 128 and 255.

  native     vilbert.functional.nce_region_loss on the gathered prediction rows (csrc/nce.hip: the index table, one pass over
             the candidate rows where they lie, backward = one scale)
  torch      BertForMultiModalPreTraining._nce_region_loss - the reference-shaped composition the model keeps as its
             fallback (and the only path before the native loss existed): index construction by B + R boolean-mask
             assignments, boolean gather of the predictions (a host sync), fancy-index gather + cat of the
             [rows, 1 + n_neg, 2048] candidates, bmm, cross entropy

The two legs draw different negatives (torch's generator / the counter-based function), so before anything is timed the
native loss and gradient are compared with the composition ON THE NATIVE LEG'S index table at the timed size. HIP events around
--iters calls after --warmup calls; every leg is measured three times, the legs alternating, and the median is reported beside
the three values. Peak memory: torch.cuda.max_memory_allocated over one call, minus what was allocated before it. Needs a GPU.

    python tools/nce_loss_bench.py [--iters 20] [--warmup 3]
"""
import argparse
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from vilbert import functional as F  # noqa: E402
from vilbert import ops  # noqa: E402
from vilbert.vilbert import BertForMultiModalPreTraining  # noqa: E402

DEV = "cuda:0"
REPEATS = 3
BATCH, REGIONS, DIM, LABELLED = 256, 36, 2048, 0.15


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters          # ms per call


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak / 2.0 ** 20


def one_shape(num_negative, args):
    n_across, n_inside = int(num_negative * 0.7), int(num_negative * 0.3)
    n_neg = n_across + n_inside
    g = torch.Generator().manual_seed(num_negative)
    labelled = (torch.rand(BATCH, REGIONS, generator=g) < LABELLED).to(DEV)
    image_target = torch.randn(BATCH, REGIONS, DIM, generator=g).to(DEV)
    scores = (torch.randn(BATCH, REGIONS, DIM, generator=g) / DIM ** 0.5).to(DEV).requires_grad_(True)
    input_ids = torch.zeros(BATCH, 36, dtype=torch.int64, device=DEV)
    idx_r = torch.nonzero(labelled.reshape(-1)).squeeze(1)
    rows = idx_r.numel()
    count = torch.full((1,), float(rows), device=DEV)
    predict = scores.detach().reshape(-1, DIM).index_select(0, idx_r).requires_grad_(True)
    stub = types.SimpleNamespace(num_negative=num_negative, vis_criterion=torch.nn.CrossEntropyLoss())

    def native():
        predict.grad = None
        loss = F.nce_region_loss(predict, image_target, idx_r, None, count, BATCH, REGIONS, n_across, n_inside, seed=77)
        loss.backward()
        return loss

    def composition():
        scores.grad = None
        loss = BertForMultiModalPreTraining._nce_region_loss(stub, input_ids, scores, image_target, labelled)
        loss.backward()
        return loss

    # same results first: the composition's arithmetic on the native leg's negatives, at this size
    neg = ops.nce_negatives(idx_r, BATCH, REGIONS, n_across, n_inside, 77)
    p2 = predict.detach().clone().requires_grad_(True)
    flat = image_target.view(BATCH * REGIONS, -1)
    sample = torch.cat((flat[idx_r].unsqueeze(1), flat[neg]), dim=1)
    want = torch.nn.functional.cross_entropy(torch.bmm(sample, p2.unsqueeze(2)).squeeze(2),
                                             torch.zeros(rows, dtype=torch.int64, device=DEV))
    want.backward()
    got = native()
    err_l = abs(got.item() - want.item())
    err_g = (predict.grad - p2.grad).abs().max().item()
    gmax = p2.grad.abs().max().item()
    assert err_l <= 1e-5 * abs(want.item()) + 1e-6 and err_g <= 1e-4 * gmax, (err_l, err_g, gmax)
    del sample, want, p2, neg
    predict.grad = None
    torch.cuda.empty_cache()

    print("num_negative %d (%d across + %d inside = %d negatives), %d labelled rows of %d, dim %d; %d calls after %d warm-up:"
          % (num_negative, n_across, n_inside, n_neg, rows, BATCH * REGIONS, DIM, args.iters, args.warmup))
    print("  same index table: |loss diff| %.2e, max |gradient diff| %.2e (max |gradient| %.2e)" % (err_l, err_g, gmax))
    fns = {"native": native, "torch": composition}
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            res[k].append(timed(fn, args.warmup, args.iters))
    med = {k: statistics.median(v) for k, v in res.items()}
    mem = {k: peak_mib(fn) for k, fn in fns.items()}
    for k in fns:
        print("  %-7s median %9.3f ms   (%s)   peak %9.1f MiB" % (k, med[k], "  ".join("%.3f" % x for x in res[k]), mem[k]))
    print("  torch / native: time %.1fx, peak memory %.1fx%s" % (
        med["torch"] / med["native"], mem["torch"] / max(mem["native"], 1e-9),
        "" if med["native"] < med["torch"] and mem["native"] < mem["torch"] else "   NATIVE IS NOT BETTER"))
    cand_bytes = rows * (1 + n_neg) * DIM * 4.0
    print("  candidate rows read per pass: %.2f GB; two passes in %.3f ms = %.2f TB/s through the caches"
          % (cand_bytes / 1e9, med["native"], 2 * cand_bytes / (med["native"] * 1e-3) / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nce_loss_bench needs a GPU - nothing is measured without one")
    for num_negative in (128, 255):
        one_shape(num_negative, args)


if __name__ == "__main__":
    main()
