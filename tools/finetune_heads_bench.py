"""Cost of the fine-tuning wrapper's heads in the bf16 training mode, at a task shape of `bench.py` (bert_base_6layer_6conect,
--tokens 24 --regions 101 --batch 128): the whole training step, the section behind the encoder alone, and the two 1-wide
logits against the launches they replace.

  step          VILBertForVLTasks forward + BCE-with-logits loss on ONE output + backward + AdamW step, dropout on, for the
                loss on `vil_prediction` and on `vision_logit`:
    all heads     every head computed (the default; on a tree without `set_active_heads` the only leg)
    one head      `set_active_heads([that output])`
  head section  everything behind the encoder, forward + backward with a gradient into all nine outputs, on fixed bf16 encoder
                outputs: `bf16 heads` (the route of this tree) against `fp32 heads` (ops16.set_heads(False): both hidden states
                cast to fp32, fp32-tensor launches - the parent's computation)
  logits        forward + backward of the two 1-wide linears over all rows: `skinny` (csrc/finetune16.hip: dropout, linear and
                region mask in one launch per pass) against `replaced` (cast + dropout + N = 1 fp32-tensor GEMM)

The script runs on a tree without the route too (legs that need it are skipped), so that two checkouts can be alternated on
one machine: their `step / all heads` lines compare directly. HIP events around --iters calls after --warmup calls; every leg
is measured three times, the legs alternating; the median is reported beside the three values. Needs a GPU.

    python tools/finetune_heads_bench.py [--batch 128] [--tokens 24] [--regions 101] [--iters 20] [--warmup 3]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import synth  # noqa: E402
from vilbert import _native, functional as F, ops, ops16, task_losses  # noqa: E402
from vilbert.optim import AdamW  # noqa: E402
from vilbert.vilbert import BertConfig, VILBertForVLTasks  # noqa: E402

DEV = "cuda:0"
REPEATS = 3
NAMES = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask", "co_attention_mask")
HEADS = ("vil_prediction", "vil_prediction_gqa", "vil_logit", "vil_binary_prediction", "vil_tri_prediction",
         "vision_prediction", "vision_logit", "linguisic_prediction", "linguisic_logit")


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


def alternate(fns, args):
    res = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            res[k].append(timed(fn, args.warmup, args.iters))
    for k in fns:
        print("  %-28s median %8.3f ms   (%s)" % (k, statistics.median(res[k]), "  ".join("%.3f" % x for x in res[k])))
    return {k: statistics.median(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--tokens", type=int, default=24)
    ap.add_argument("--regions", type=int, default=101)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="bert_base_6layer_6conect.json")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_heads_bench needs a GPU - nothing is measured without one")
    _native.set_gemm_mode("bf16")
    B, T, R = args.batch, args.tokens, args.regions
    cfg = synth.load_config(args.config)
    m = VILBertForVLTasks(BertConfig.from_dict(cfg), num_labels=1).to(DEV).train()
    has_selection = hasattr(m, "set_active_heads")
    has_route = has_selection and hasattr(ops16, "skinny_fwd") and m._bf16_heads_ok()
    x = synth.make_inputs(cfg, B, T, R)
    inputs = [x[n].to(DEV) for n in NAMES]
    opt = AdamW(m.parameters(), lr=1e-5, weight_decay=0.01)
    bce = task_losses.BCEWithLogitsLoss(reduction="mean")
    g = torch.Generator().manual_seed(1)
    print("%s, batch %d, %d tokens, %d regions (%d text rows, %d region rows); head selection %s, bf16 route %s"
          % (args.config, B, T, R, B * T, B * R, "yes" if has_selection else "NO (all heads only)", "yes" if has_route else "NO"))

    # ---- the whole step ---------------------------------------------------------------------------------------------------
    with torch.no_grad():
        shapes = [tuple(o.shape) for o in m(*inputs)[:9]]
    targets = {n: torch.rand(shapes[HEADS.index(n)], generator=g).to(DEV) for n in ("vil_prediction", "vision_logit")}

    def step(name, selected):
        def run():
            if has_selection:
                m.set_active_heads([name] if selected else None)
            opt.zero_grad()
            loss = bce(m(*inputs)[HEADS.index(name)], targets[name])
            loss.backward()
            opt.step()
            return loss
        return run
    for name in ("vil_prediction", "vision_logit"):
        print("training step, BCE loss on %s; %d calls after %d warm-up:" % (name, args.iters, args.warmup))
        fns = {"step / all heads": step(name, False)}
        if has_selection:
            fns["step / one head"] = step(name, True)
        med = alternate(fns, args)
        if has_selection:
            print("  all heads / one head: %.2fx" % (med["step / all heads"] / med["step / one head"]))
    if has_selection:
        m.set_active_heads(None)
    if not has_route:
        return

    # ---- the head section alone, on fixed bf16 encoder outputs ---------------------------------------------------------------
    seq_t = torch.randn(B, T, cfg["hidden_size"], generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    seq_v = torch.randn(B, R, cfg["v_hidden_size"], generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    bert = m.bert

    def fake_encoder(*_a, **_k):
        if bert.__dict__.pop("_bf16_seq_out", False):
            return seq_t, seq_v, None, None, None
        t32, v32 = F.to_f32(seq_t), F.to_f32(seq_v)
        return t32, v32, bert.t_pooler(t32), bert.v_pooler(v32), None
    grads = [torch.randn(s, generator=g).to(DEV) for s in shapes]

    def head_section(bf16_heads):
        def run():
            prev = ops16.set_heads(bf16_heads)
            try:
                for p in m.parameters():
                    p.grad = None
                seq_t.grad = seq_v.grad = None
                out = m(*inputs)[:9]
                torch.autograd.backward(out, grads)
            finally:
                ops16.set_heads(prev)
        return run
    bert.forward = fake_encoder
    try:
        print("head section alone (all nine heads), forward + backward:")
        med = alternate({"bf16 heads": head_section(True), "fp32 heads": head_section(False)}, args)
        print("  fp32 heads / bf16 heads: %.2fx%s" % (med["fp32 heads"] / med["bf16 heads"],
                                                      "" if med["bf16 heads"] <= med["fp32 heads"] else "   THE NEW PATH IS SLOWER"))
        for name in ("vil_prediction", "vision_logit"):
            m.set_active_heads([name])
            i = HEADS.index(name)

            def one(bf16_heads, i=i):
                def run():
                    prev = ops16.set_heads(bf16_heads)
                    try:
                        for p in m.parameters():
                            p.grad = None
                        seq_t.grad = seq_v.grad = None
                        m(*inputs)[i].backward(grads[i])
                    finally:
                        ops16.set_heads(prev)
                return run
            print("head section alone, %s selected, forward + backward:" % name)
            alternate({"bf16 heads": one(True), "fp32 heads": one(False)}, args)
        m.set_active_heads(None)
    finally:
        del bert.forward

    # ---- the two 1-wide logits against what they replace ---------------------------------------------------------------------
    p = m.dropout.p
    mask = ops.additive_mask(inputs[5])

    def logits(skinny):
        def run():
            for lin in (m.vision_logit, m.linguisic_logit):
                lin.weight.grad = lin.bias.grad = None
            seq_t.grad = seq_v.grad = None
            if skinny:
                v = F.skinny_linear(seq_v, m.vision_logit.weight, m.vision_logit.bias, row_add=mask, drop_p=p)
                t = F.skinny_linear(seq_t, m.linguisic_logit.weight, m.linguisic_logit.bias, drop_p=p)
            else:
                v = F.linear(F.dropout(F.to_f32(seq_v), p), m.vision_logit.weight, m.vision_logit.bias, residual=mask.unsqueeze(2))
                t = F.linear(F.dropout(F.to_f32(seq_t), p), m.linguisic_logit.weight, m.linguisic_logit.bias)
            torch.autograd.backward([v, t], [grads[6], grads[8]])
        return run
    print("vision_logit + linguisic_logit, forward + backward (p = %.2f):" % p)
    med = alternate({"skinny": logits(True), "replaced": logits(False)}, args)
    print("  replaced / skinny: %.2fx%s" % (med["replaced"] / med["skinny"],
                                            "" if med["skinny"] <= med["replaced"] else "   THE SKINNY KERNELS ARE SLOWER"))


if __name__ == "__main__":
    main()
