"""Cost of the native LAMB step (vilbert.optim.LAMB: norm pass + two launches, csrc/lamb.hip) on the parameters of the tiny and
of the base 6-layer / 6-connection pre-training model, against

  clipped AdamW   vilbert.optim.AdamW(max_grad_norm=1.0).step() on the same parameters: norm pass + scaled update, 4 + 28 = 32 B
                  per parameter. LAMB moves 4 + 24 + 16 = 44 B, so the derived target is LAMB / AdamW <= 44 / 32 = 1.375, with 10 %
                  on top for one more launch and box-to-box spread: 1.5125.
  torch loop      LAMB restated as a per-tensor loop of torch operations that keeps every scalar on the device (no host read:
                  the arithmetic of tests/lamb_restatement.py, which reads its norms back and would measure the synchronisations)

HIP events around windows of --iters steps after a warm-up; the variants alternate inside every round, so that drift of the
machine hits all of them alike; per variant the median window, the fastest and the slowest are printed, and the AdamW step is
timed twice per round: the difference between the two is the run-to-run spread a difference has to exceed. Bytes are
algorithmic (from the shapes), rates are bytes / median time. Needs a GPU; prints the register / scratch figures the build
recorded for the two kernels.

    python tools/lamb_step_bench.py [--rounds 7] [--iters 20] > profiles/lamb_step_ab.txt
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
from oracle import synth  # noqa: E402
from vilbert import _native as N  # noqa: E402
from vilbert.optim import AdamW, CHUNK_ELEMS, LAMB  # noqa: E402

DEV = "cuda:0"
TARGET = 44.0 / 32.0 * 1.10


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / iters          # us per call


class LoopLAMB(object):
    """The defaults of vilbert.optim.LAMB (decoupled decay, bias correction, gradient averaging, max_grad_norm = 1) as a loop
    over the tensors; the clip coefficient and the trust ratios stay device scalars."""

    def __init__(self, params, lr, weight_decay, betas=(0.9, 0.999), eps=1e-6, max_grad_norm=1.0):
        self.params, self.lr, self.wd, self.betas, self.eps, self.max_norm = params, lr, weight_decay, betas, eps, max_grad_norm
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.t = 0
        self.one = torch.ones((), device=params[0].device)

    @torch.no_grad()
    def step(self):
        beta1, beta2 = self.betas
        self.t += 1
        bc1, bc2 = 1.0 - beta1 ** self.t, 1.0 - beta2 ** self.t
        norm = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in self.params]))
        coef = torch.clamp(self.max_norm / (norm + 1e-6), max=1.0)
        for p, m, v, wd in zip(self.params, self.m, self.v, self.wd):
            g = p.grad * coef
            m.mul_(beta1).add_(g, alpha=1.0 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
            u = (m / bc1) / ((v / bc2).sqrt_().add_(self.eps))
            if wd != 0.0:
                u.add_(p, alpha=wd)
                pn, un = torch.linalg.vector_norm(p), torch.linalg.vector_norm(u)
                r = torch.where((pn > 0) & (un > 0), pn / un, self.one)
                p.sub_(u * (r * self.lr))
            else:
                p.sub_(u, alpha=self.lr)


def bench(label, cfg, args):
    from vilbert import arena as A
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    torch.manual_seed(0)
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfg)).to(DEV)
    params = [p for p in model.parameters() if p.requires_grad]
    n = sum(p.numel() for p in params)
    groups = lambda: [{"params": [p], "weight_decay": 0.01 if p.dim() > 1 else 0.0} for p in params]
    adamw = AdamW(groups(), lr=1e-5, correct_bias=False, max_grad_norm=1.0)
    arena = adamw._arena
    native = LAMB(groups(), lr=1e-4, max_grad_norm=1.0)
    loop = LoopLAMB(params, 1e-4, [0.01 if p.dim() > 1 else 0.0 for p in params])
    arena.flat.normal_(0.0, 1e-3)
    for p in params:
        p.grad = arena.alias(A.lookup(p)[1])
    variants = [("clipped AdamW", adamw.step, 32), ("clipped AdamW again", adamw.step, 32), ("native LAMB (this)", native.step, 44),
                ("LAMB torch loop", loop.step, None)]
    for _name, fn, _b in variants:              # warm-up: plans, state, code objects
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _fn, _b in variants}
    for _ in range(args.rounds):
        for name, fn, _b in variants:
            times[name].append(window(fn, args.iters))
    print("%s: %d tensors, %.1f M parameters, %d chunks of %d; %d rounds x %d calls after %d warm-up calls, variants alternating"
          % (label, len(params), n / 1e6, native._plan["n_chunks"], CHUNK_ELEMS, args.rounds, args.iters, args.warmup))
    print("  %-22s %10s %10s %10s %8s %8s" % ("variant", "median us", "min us", "max us", "B/param", "TB/s"))
    med = {}
    for name, _fn, nbytes in variants:
        t = times[name]
        med[name] = statistics.median(t)
        rate = "%8d %8.2f" % (nbytes, nbytes * n / med[name] / 1e6) if nbytes else "%8s %8s" % ("-", "-")
        print("  %-22s %10.1f %10.1f %10.1f %s" % (name, med[name], min(t), max(t), rate))
    ratio = med["native LAMB (this)"] / med["clipped AdamW"]
    print("  run-to-run spread (AdamW vs AdamW again, medians): %.2f %%" % (100 * abs(med["clipped AdamW"] - med["clipped AdamW again"]) / med["clipped AdamW"]))
    print("  native LAMB / clipped AdamW = %.3f (derived target <= %.4f: %s)   torch loop / native LAMB = %.1f"
          % (ratio, TARGET, "met" if ratio <= TARGET else "MISSED", med["LAMB torch loop"] / med["native LAMB (this)"]))
    print("  grad_norm %.6f  skipped steps %d  trust ratios %.4f .. %.4f" % (native.grad_norm.item(), native.skipped_steps(),
                                                                            native.trust_ratios.min().item(), native.trust_ratios.max().item()))
    del model, adamw, native, loop, arena
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lamb_step_bench needs a GPU - nothing is measured without one")
    bench("tiny", synth.tiny_config(), args)
    bench("bert_base_6layer_6conect", synth.load_config("bert_base_6layer_6conect.json"), args)
    for name in ("lamb", "optimizer"):
        res = os.path.join(os.path.dirname(N.LIB_PATH), name + ".resource.txt")
        if os.path.isfile(res):
            for fn, sg, vg, sc, occ in re.findall(r"Function Name: (\S+).*?TotalSGPRs: (\d+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)"
                                                  r".*?Occupancy \[waves/SIMD\]: (\d+)", open(res).read(), flags=re.S):
                print("kernel %s: %s VGPRs, %s SGPRs, scratch %s B/lane, %s waves/SIMD" % (fn, vg, sg, sc, occ))


if __name__ == "__main__":
    main()
