"""Cost of the fine-tuning loss and answer score (task_utils.py:325-374, 618-623 of the reference) on the two head shapes
that matter - the 3,129-way answer head at the VQA batch and the binary head - and inside a whole fine-tuning step:

  native           vilbert.task_losses: BCEWithLogitsLoss (csrc/task_loss.hip: one reduction forward, one launch backward)
                   and compute_score_with_logits (one launch)
  torch            the reference's sequence: nn.BCEWithLogitsLoss(reduction="mean"), and max / zeros / scatter_ / mul for the
                   score
  isolated         criterion(x, t).mean() * t.size(1), backward into x, score(x, t).sum() / batch - on fixed tensors
  whole step       VILBertForVLTasks (bert_base_6layer_6conect.json) forward + that loss and score + backward + AdamW at
                   batch 128 / 23 tokens / 101 regions, with each of the two

HIP events around --iters calls after --warmup calls; every leg is measured three times, the two legs alternating, and the
median is reported beside the three values. Needs a GPU.

    python tools/task_loss_bench.py [--iters 200] [--warmup 20] [--step-iters 10] [--step-warmup 3]
"""
import argparse
import os
import statistics
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import synth  # noqa: E402
from vilbert import task_losses as TL  # noqa: E402
from vilbert.optim import AdamW  # noqa: E402
from vilbert.vilbert import BertConfig, VILBertForVLTasks  # noqa: E402

DEV = "cuda:0"
NAMES = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask")
REPEATS = 3


def upstream_score(logits, labels):
    """compute_score_with_logits as the reference writes it."""
    logits = torch.max(logits, 1)[1].data
    one_hots = torch.zeros(*labels.size()).cuda()
    one_hots.scatter_(1, logits.view(-1, 1), 1)
    return one_hots * labels


LEGS = {"native": (TL.BCEWithLogitsLoss(reduction="mean"), TL.compute_score_with_logits),
        "torch": (nn.BCEWithLogitsLoss(reduction="mean"), upstream_score)}


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


def alternate(fns, warmup, iters):
    """{leg: [ms] * REPEATS}, the legs taking turns so that a drift of the machine hits both."""
    out = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            out[k].append(timed(fn, warmup, iters))
    return out


def report(label, unit, res):
    med = {k: statistics.median(v) for k, v in res.items()}
    for k, v in res.items():
        print("  %-22s %-7s median %9.4f %s   (%s)" % (label, k, med[k], unit, "  ".join("%.4f" % x for x in v)))
    print("  %-22s torch / native = %.2f%s" % (label, med["torch"] / med["native"],
                                              "" if med["native"] <= med["torch"] else "   NATIVE IS SLOWER"))
    return med


def isolated(shape, args):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g).to(DEV).requires_grad_(True)
    t = torch.zeros(*shape)
    t[torch.arange(shape[0]), torch.randint(0, shape[1], (shape[0],), generator=g)] = 1.0
    t = t.to(DEV)

    def leg(crit, score):
        def fn():
            x.grad = None
            loss = crit(x, t).mean() * t.size(1)
            loss.backward()
            return loss, score(x, t).sum() / float(shape[0])
        return fn
    fns = {k: leg(*v) for k, v in LEGS.items()}
    (ln, sn), (lt, st) = fns["native"](), fns["torch"]()
    assert abs(ln.item() - lt.item()) <= 1e-5 * abs(lt.item()) and sn.item() == st.item()
    print("loss forward + backward + score on [%d, %d], %d calls after %d warm-up:" % (shape + (args.iters, args.warmup)))
    report("isolated", "ms", alternate(fns, args.warmup, args.iters))


def whole_step(args):
    cfg = synth.load_config("bert_base_6layer_6conect.json")
    batch, n_tok, n_reg = 128, 23, 101
    torch.manual_seed(0)
    net = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=3129).to(DEV).train()
    no_decay = ("bias", "LayerNorm.bias", "LayerNorm.weight")
    optim = AdamW([{"params": [p for n, p in net.named_parameters() if not any(k in n for k in no_decay)], "weight_decay": 0.01},
                   {"params": [p for n, p in net.named_parameters() if any(k in n for k in no_decay)], "weight_decay": 0.0}],
                  lr=4e-5)
    x = synth.make_inputs(cfg, batch, n_tok, n_reg)
    inp = [x[n].to(DEV) for n in NAMES]
    g = torch.Generator().manual_seed(11)
    target = torch.zeros(batch, 3129)
    target[torch.arange(batch), torch.randint(0, 3129, (batch,), generator=g)] = 1.0
    target = target.to(DEV)

    def leg(crit, score):
        def fn():
            optim.zero_grad(set_to_none=True)
            pred = net(*inp)[0]
            loss = crit(pred, target).mean() * target.size(1)
            batch_score = score(pred, target).sum() / float(batch)
            loss.backward()
            optim.step()
            return loss, batch_score
        return fn
    fns = {k: leg(*v) for k, v in LEGS.items()}
    print("VILBertForVLTasks step (bert_base_6layer_6conect, batch %d / %d tokens / %d regions, forward + loss + score + "
          "backward + AdamW, dropout on), %d steps after %d warm-up:" % (batch, n_tok, n_reg, args.step_iters, args.step_warmup))
    med = report("whole step", "ms", alternate(fns, args.step_warmup, args.step_iters))
    print("  whole step             native - torch = %+.4f ms" % (med["native"] - med["torch"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=10)
    ap.add_argument("--step-warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("task_loss_bench needs a GPU - nothing is measured without one")
    isolated((128, 3129), args)
    isolated((256, 2), args)
    whole_step(args)


if __name__ == "__main__":
    main()
