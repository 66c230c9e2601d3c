"""Cost of the RAdam step (`train_tasks.py --optim RAdam`) on the tiny and the base 6-layer model, one parameter group per
tensor as train_tasks.py builds them:

  native step      vilbert.optim.RAdam.step(): ONE launch over all tensors (csrc/optimizer.hip: radam_kernel)
  torch loop       the reference's step restated as a per-tensor loop of torch operations (tests/radam_restatement.py; about
                   nine small launches per tensor - the reference's own class is not present where the GPU is)
  whole step       VILBertForVLTasks forward + loss + backward + optimizer step, with each of the two

HIP events around --iters steps after --warmup steps, on gradients that stay fixed (the optimizer step alone) or on a fixed
batch (the whole step). Needs a GPU.

    python tools/radam_step_bench.py [--iters 20] [--warmup 5] [--batch 8]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import radam_restatement as rr  # noqa: E402
from oracle import synth  # noqa: E402
from vilbert.optim import RAdam  # noqa: E402
from vilbert.vilbert import BertConfig, VILBertForVLTasks  # noqa: E402

DEV = "cuda:0"
NAMES = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "co_attention_mask")


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


class LoopRAdam(object):
    """The restated per-tensor loop behind the two calls the training loop makes."""

    def __init__(self, params, lr):
        self.params = params
        self.r = rr.Restatement([p.data for p in params], [{"idx": [i], "lr": lr, "weight_decay": 0.01 if p.dim() > 1 else 0.0}
                                                           for i, p in enumerate(params)], clone=False)

    def step(self):
        self.r.step([p.grad for p in self.params])

    def zero_grad(self):
        for p in self.params:
            p.grad = None


def model_and_batch(cfg, batch):
    model = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1).to(DEV).train()
    x = synth.make_inputs(cfg, batch, 20, 37)
    return model, [x[n].to(DEV) for n in NAMES]


def bench(label, cfg, args):
    lr = 4e-5
    rows = []
    for kind in ("native", "loop"):
        torch.manual_seed(0)
        model, inputs = model_and_batch(cfg, args.batch)
        params = [p for p in model.parameters() if p.requires_grad]
        if kind == "native":
            opt = RAdam([{"params": [p], "lr": lr, "weight_decay": 0.01 if p.dim() > 1 else 0.0} for p in params], lr=lr)
        else:
            opt = LoopRAdam(params, lr)

        def whole():
            opt.zero_grad()
            out = model(*inputs)
            loss = out[0].float().pow(2).mean() + out[2].float().pow(2).mean()
            loss.backward()
            opt.step()
        whole_ms = timed(whole, args.warmup, args.iters)
        with_grad = [p for p in params if p.grad is not None]
        step_ms = timed(opt.step, args.warmup, args.iters)          # the gradients of the last backward stay in place
        rows.append((kind, len(with_grad), sum(p.numel() for p in with_grad), step_ms, whole_ms))
        del model, opt
        torch.cuda.empty_cache()
    (_, n_t, n_e, nat_step, nat_whole), (_, _, _, loop_step, loop_whole) = rows
    print("%s: %d tensors with a gradient, %.1f M elements, batch %d, %d steps after %d warm-up"
          % (label, n_t, n_e / 1e6, args.batch, args.iters, args.warmup))
    print("  optimizer step alone   native %9.3f ms   torch loop %9.3f ms   loop / native = %.1f"
          % (nat_step, loop_step, loop_step / nat_step))
    print("  whole training step    native %9.3f ms   torch loop %9.3f ms   loop / native = %.2f"
          % (nat_whole, loop_whole, loop_whole / nat_whole))
    print("  native step: %.0f GB/s of the 28 B per element it moves" % (28.0 * n_e / nat_step / 1e6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("radam_step_bench needs a GPU - nothing is measured without one")
    bench("tiny", synth.tiny_config(), args)
    bench("bert_base_6layer_6conect", synth.load_config("bert_base_6layer_6conect.json"), args)


if __name__ == "__main__":
    main()
