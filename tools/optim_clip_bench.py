"""A/B of the optimizer step with global-norm clipping on the base model's parameters (bert_base_6layer_6conect, ~250 M):

  plain        vilbert.optim.AdamW.step() with the defaults (vb_adamw_step, 28 B per parameter)
  clipped      AdamW(max_grad_norm=1.0, skip_nonfinite=True).step(): norm pass + scaled update (28 + 4 B per parameter)
  torch clip   what FusedAdam.step() did before: torch.linalg.vector_norm(arena.flat), flat.mul_(coef), then the plain step
               (28 + 12 B per parameter)
  norm pass    vbx_grad_norm alone (4 B per parameter)

HIP events around windows of --iters steps after a warm-up; the variants alternate inside every round, so that drift of the
machine hits all of them alike; per variant the median window, the fastest and the slowest are printed, and plain is timed
twice per round (plain / plain again): the difference between the two is the run-to-run spread a difference has to exceed.
Bytes are algorithmic (from the shapes), rates are bytes / median time. Needs a GPU; prints the register / scratch figures
the build recorded for the optimizer kernels.

    python tools/optim_clip_bench.py [--rounds 7] [--iters 20] [--config bert_base_6layer_6conect.json]
"""
import argparse
import os
import re
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from vilbert import _native as N  # noqa: E402
from vilbert.optim import AdamW, CHUNK_ELEMS  # noqa: E402

DEV = "cuda:0"


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--config", default="bert_base_6layer_6conect.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_clip_bench needs a GPU - nothing is measured without one")
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "vilbert-multi-task_amd", "config", args.config))
    model = BertForMultiModalPreTraining(cfg).to(DEV)
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)

    plain = AdamW(params, lr=1e-5, correct_bias=False)
    arena = plain._arena
    clipped = AdamW(params, lr=1e-5, correct_bias=False, max_grad_norm=1.0, skip_nonfinite=True)
    legacy = AdamW(params, lr=1e-5, correct_bias=False)
    torch.manual_seed(0)
    arena.flat.normal_(0.0, 1e-3)
    from vilbert import arena as A
    for p in params:
        p.grad = arena.alias(A.lookup(p)[1])

    def torch_clip_step():
        flat = arena.flat
        norm = torch.linalg.vector_norm(flat)
        flat.mul_(torch.clamp(1.0 / (norm + 1e-6), max=1.0))
        legacy.step()

    def norm_only():
        plan = clipped._plan
        N.check(N.lib().vbx_grad_norm(N.stream_ptr(), plan["n_chunks"], plan["dev_tab"].data_ptr(),
                                      plan["chunk_tensor"].data_ptr(), plan["chunk_off"].data_ptr(), CHUNK_ELEMS, 1.0, 1.0, 1,
                                      plan["partials"].data_ptr(), clipped._grad_state.data_ptr()), "vbx_grad_norm")

    variants = [("plain", plain.step, 28), ("plain again", plain.step, 28), ("clipped (this)", clipped.step, 32),
                ("torch clip + plain", torch_clip_step, 40), ("norm pass alone", norm_only, 4)]
    for _name, fn, _b in variants:              # warm-up: plans, state, code objects
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _fn, _b in variants}
    for _ in range(args.rounds):
        for name, fn, _b in variants:
            times[name].append(window(fn, args.iters))
    print("optimizer step on %s: %d tensors, %.1f M parameters, %d chunks of %d; %d rounds x %d calls, variants alternating"
          % (args.config, len(params), n / 1e6, clipped._plan["n_chunks"], CHUNK_ELEMS, args.rounds, args.iters))
    print("%-20s %10s %10s %10s %8s %8s" % ("variant", "median us", "min us", "max us", "B/param", "TB/s"))
    med = {}
    for name, _fn, nbytes in variants:
        t = times[name]
        med[name] = statistics.median(t)
        print("%-20s %10.1f %10.1f %10.1f %8d %8.2f" % (name, med[name], min(t), max(t), nbytes, nbytes * n / med[name] / 1e6))
    spread = abs(med["plain"] - med["plain again"]) / med["plain"]
    print("run-to-run spread (plain vs plain again, medians): %.2f %%" % (100 * spread))
    print("clipped / (torch clip + plain) = %.3f   clipped - plain = %.1f us   norm pass alone = %.1f us"
          % (med["clipped (this)"] / med["torch clip + plain"], med["clipped (this)"] - med["plain"], med["norm pass alone"]))
    print("grad_norm %.6f  skipped steps %d" % (clipped.grad_norm.item(), clipped.skipped_steps()))
    res = os.path.join(os.path.dirname(N.LIB_PATH), "optimizer.resource.txt")
    if os.path.isfile(res):
        for fn, sg, vg, sc in re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)",
                                         open(res).read(), flags=re.S):
            print("kernel %s: %s VGPRs, %s SGPRs, scratch %s B/lane" % (fn, vg, sg, sc))


if __name__ == "__main__":
    main()
