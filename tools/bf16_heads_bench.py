"""Cost of everything behind the encoder in the bf16 training mode - poolers, prediction heads, the three losses - alone,
forward + backward, at the row counts of `bench.py --gemm-mode bf16` (bert_base_6layer_6conect, T = 36, R = 37, ~15 % of the
positions labelled, fixed-capacity gather at 0.25), and of the MLM decoder's input gradient in its three forms.

  bf16 heads  BertForMultiModalPreTraining._losses_on_the_bf16_stream on the encoder's bf16 outputs (csrc/heads16.hip: one
              gather per stream, bf16 GEMMs on zero-padded decoder shadows, bf16 loss gradients, one scatter per stream)
  fp32 heads  what VB_BF16_HEADS=0 runs: both hidden states cast to fp32 (and their gradients back), then the fp32-tensor
              kernels of this mode (_losses_at_labelled_positions)

  dX of the 30,522-wide decoder, rows x 30,720 -> rows x 768:
  dgrad form  vb_linear_bf16 on the transposed padded shadow (one persistent launch, about 6 output tiles per 256 rows)
  wgrad form  vb_wgrad_bf16 on G^T and the padded shadow (contraction splits from its planner) + one cast
  fp32 tensor ops.linear_bwd_input on the fp32 gradient (the launch the bf16 forms replace)

HIP events around --iters calls after --warmup calls; every leg is measured three times, the legs alternating; the median is
reported beside the three values. Losses of the two head legs are printed side by side first. Needs a GPU.

    python tools/bf16_heads_bench.py [--batch 256] [--iters 20] [--warmup 3]
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
from vilbert import _native, functional as F, ops, ops16  # noqa: E402
from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining  # noqa: E402

DEV = "cuda:0"
REPEATS = 3
T, R = 36, 37


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
        print("  %-11s median %8.3f ms   (%s)" % (k, statistics.median(res[k]), "  ".join("%.3f" % x for x in res[k])))
    return {k: statistics.median(v) for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_heads_bench needs a GPU - nothing is measured without one")
    _native.set_gemm_mode("bf16")
    B = args.batch
    cfg = synth.load_config("bert_base_6layer_6conect.json")
    m = BertForMultiModalPreTraining(BertConfig.from_dict(cfg)).to(DEV).train()
    m.label_capacity = 0.25
    x = synth.make_inputs(cfg, B, T, R, with_labels=True)
    lab = [x[n].to(DEV) for n in ("masked_lm_labels", "image_label", "image_target", "next_sentence_label")]
    g = torch.Generator().manual_seed(1)
    seq_t = torch.randn(B, T, cfg["hidden_size"], generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    seq_v = torch.randn(B, R, cfg["v_hidden_size"], generator=g).to(torch.bfloat16).to(DEV).requires_grad_(True)
    assert m._bf16_heads_ok()

    def run(losses):
        for p in m.parameters():
            p.grad = None
        seq_t.grad = seq_v.grad = None
        sum(l.sum() for l in losses).backward()
        return [l.item() for l in losses] if run.report else None
    run.report = False

    def bf16_heads():
        return run(m._losses_on_the_bf16_stream(seq_t, seq_v, *lab))

    def fp32_heads():
        t32, v32 = F.to_f32(seq_t), F.to_f32(seq_v)
        return run(m._losses_at_labelled_positions(t32, v32, m.bert.t_pooler(t32), m.bert.v_pooler(v32), *lab))

    run.report = True
    print("batch %d: %d text rows, %d region rows; losses bf16 heads %s, fp32 heads %s"
          % (B, B * T, B * R, ["%.5f" % v for v in bf16_heads()], ["%.5f" % v for v in fp32_heads()]))
    run.report = False
    print("heads + losses, forward + backward; %d calls after %d warm-up:" % (args.iters, args.warmup))
    med = alternate({"bf16 heads": bf16_heads, "fp32 heads": fp32_heads}, args)
    print("  fp32 heads / bf16 heads: %.2fx%s" % (med["fp32 heads"] / med["bf16 heads"],
                                                  "" if med["bf16 heads"] <= med["fp32 heads"] else "   THE NEW PATH IS SLOWER"))

    # the MLM decoder's input gradient
    w, b = m.cls.predictions.decoder.weight, m.cls.predictions.bias
    n, K = w.shape
    rows = max(32, (int(B * T * 0.25) + 31) // 32 * 32)
    logits = (torch.randn(rows, (n + 3) // 4 * 4, generator=g) * 2).to(DEV)[:, :n]      # 16-byte aligned rows, as pad_cols gives
    labels = torch.randint(0, n, (rows,), generator=g).to(DEV)
    labels[int(rows * 0.6):] = -1                                       # (the padding rows of the fixed-capacity gather)
    with torch.no_grad():
        _loss, lse, count = ops.xent_fwd(logits, labels, -1)
        one = torch.ones(1, device=DEV)
        G, GT = ops16.xent_bwd16(one, logits, labels, -1, lse, count, True)
        d32 = ops.xent_bwd(one, logits, labels, -1, lse, count)
        fns = {"dgrad form": lambda: ops16.linear_ragged_bwd_input(G, GT, w, b, rows, form="dgrad"),
               "wgrad form": lambda: ops16.linear_ragged_bwd_input(G, GT, w, b, rows, form="wgrad"),
               "fp32 tensor": lambda: ops.linear_bwd_input(d32, [w], K)}
        a, c = fns["dgrad form"]().float(), fns["wgrad form"]().float()
        ref = fns["fp32 tensor"]()
        print("dX of the %d-wide decoder, %d rows (n_pad %d, m_pad %d): relative L2 against the fp32-tensor launch - dgrad "
              "form %.2e, wgrad form %.2e" % (n, rows, G.shape[1], GT.shape[1], ((a - ref).norm() / ref.norm()).item(),
                                              ((c - ref).norm() / ref.norm()).item()))
        med = alternate(fns, args)
    print("  switch width (ops16.WGRAD_FORM_MIN_WIDTH = %d): the wgrad form is %s here"
          % (ops16.WGRAD_FORM_MIN_WIDTH, "the faster bf16 form" if med["wgrad form"] < med["dgrad form"] else "NOT the faster bf16 form"))


if __name__ == "__main__":
    main()
