"""Cost of the single-stream baseline's embedding (csrc/joint_embed.hip) against the route the existing kernels offer, forward
and backward, at the two shapes that matter: (128, 38, 101, 768) - the fine-tuning task shape - and (256, 36, 37, 768).

  A  existing route   vb_text_embed_ln_fwd + vb_image_embed_ln_fwd, torch.cat of the two states and of the two additive
                      masks (two vb_additive_mask launches); backward: the two slices of the joint gradient made contiguous,
                      then vb_layernorm_bwd once per segment
  B  joint kernels    vbb_joint_embed_fwd; backward: vbb_joint_embed_bwd

Both routes end in the same tensors (checked before anything is timed). What follows the LayerNorm backward - the table
scatter, the weight-gradient GEMMs - is the same launches on the same contiguous dx buffers in both routes and is left out.
Every call works on its own set of buffers, SETS of them rotating so that a call's operands are not in the 256 MB Infinity
Cache from the call before; HIP events around --iters calls after --warmup calls, each leg three times, the legs alternating;
the median is reported beside the three values. Bytes: what the algorithm has to move, counted from the shapes below.
Needs a GPU.

    python tools/joint_embed_bench.py [--iters 60] [--warmup 10] [--step]
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
from vilbert import ops  # noqa: E402

DEV = "cuda:0"
SHAPES = [(128, 38, 101, 768), (256, 36, 37, 768)]
VOCAB, N_POS, N_TYPES = 30522, 512, 2
REPEATS = 3
CACHE_BYTES = 256 << 20


def make_set(B, T, R, H, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)
    return dict(ids=torch.randint(0, VOCAB, (B, T), generator=g).to(DEV), seg=torch.randint(0, 2, (B, T), generator=g).to(DEV),
                word=r(VOCAB, H), pos=r(N_POS, H), typ=r(N_TYPES, H), gt=r(H), bt=r(H), proj=r(B, R, H),
                loc=torch.rand(B, R, 5, generator=g).to(DEV), wl=r(H, 5), bl=r(H), typ_v=r(N_TYPES, H), gv=r(H), bv=r(H),
                mask_t=torch.randint(0, 2, (B, T), generator=g).to(DEV), mask_v=torch.randint(0, 2, (B, R), generator=g).to(DEV),
                dy=r(B, T + R, H))


def fwd_a(s):
    """The existing kernels. The image kernel has no token-type row: it is folded into the location bias for this leg."""
    t, tm, tr, tp = ops.text_embed_ln_fwd(s["ids"], s["seg"], s["word"], s["pos"], s["typ"], s["gt"], s["bt"], 1e-12, want_stats=True)
    v, vm, vr, vp = ops.image_embed_ln_fwd(s["proj"], s["loc"], s["wl"], s["bl_row"], s["gv"], s["bv"], 1e-12, want_stats=True)
    mask = torch.cat([ops.additive_mask(s["mask_t"]), ops.additive_mask(s["mask_v"])], 1)
    return torch.cat([t, v], 1), mask, (tp, tm, tr, vp, vm, vr)


def bwd_a(s, saved):
    tp, tm, tr, vp, vm, vr = saved
    T = tp.shape[1]
    dy_t, dy_v = s["dy"][:, :T].contiguous(), s["dy"][:, T:].contiguous()
    return ops.layernorm_bwd(dy_t, tp, tm, tr, s["gt"]) + ops.layernorm_bwd(dy_v, vp, vm, vr, s["gv"])


def fwd_b(s):
    out, mask, mean, rstd, presum = ops.joint_embed(s["ids"], s["seg"], s["word"], s["pos"], s["typ"], s["gt"], s["bt"], s["proj"],
                                                    s["loc"], s["wl"], s["bl"], s["typ_v"][1], s["gv"], s["bv"], 1e-12,
                                                    s["mask_t"], s["mask_v"], want_stats=True)
    return out, mask, (presum, mean, rstd)


def bwd_b(s, saved):
    presum, mean, rstd = saved
    return ops.joint_embed_bwd(s["dy"], presum, mean, rstd, s["gt"], s["gv"], s["ids"].shape[1])


def timed(fn, sets, warmup, iters):
    for i in range(warmup):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3          # us per call


def alternate(fns, sets, warmup, iters):
    out = {k: [] for k in fns}
    for _ in range(REPEATS):
        for k, fn in fns.items():
            out[k].append(timed(fn, sets, warmup, iters))
    return out


def bytes_moved(B, T, R, H):
    """Floats x 4 the two routes have to move (tables and per-row scalars left out: the same in both, and small)."""
    S = T + R
    state = B * S * H * 4
    fwd_common = B * T * H * 4 * 1 + B * R * H * 4 + 2 * state           # gathered word rows + projected features in; out + presum out
    bwd_common = 3 * state                                                # dy, presum in; dx out
    return {"fwd A": fwd_common + 2 * state, "fwd B": fwd_common,        # A: the cat reads and writes the state once more
            "bwd A": bwd_common + 2 * state, "bwd B": bwd_common}       # A: the two slices read and write the gradient once more


def check_same(s):
    oa, ma, sa = fwd_a(s)
    ob, mb, sb = fwd_b(s)
    assert torch.equal(ma, mb), "masks differ"
    assert float((oa - ob).abs().max()) <= 2e-5 * max(1.0, float(oa.abs().max())), "states differ"
    ga, gb = bwd_a(s, sa), bwd_b(s, sb)
    dx_t, dg_t, db_t, dx_v, dg_v, db_v = ga
    for a, b, n in ((dx_t, gb[0], "dx_text"), (dx_v, gb[1], "dx_img"), (dg_t, gb[2], "dgamma_t"), (db_t, gb[3], "dbeta_t"),
                    (dg_v, gb[4], "dgamma_v"), (db_v, gb[5], "dbeta_v")):
        a = a.reshape(b.shape)
        assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(a.abs().max())), n


def bench_shape(B, T, R, H, args):
    one = sum(t.numel() * t.element_size() for t in make_set(B, T, R, H, 0).values())
    n_sets = max(2, min(8, CACHE_BYTES // max(1, one - VOCAB * H * 4) + 2))
    sets = [make_set(B, T, R, H, k) for k in range(n_sets)]
    for s in sets:
        s["bl_row"] = s["bl"] + s["typ_v"][1]
    check_same(sets[0])
    saved_a = [fwd_a(s)[2] for s in sets]
    saved_b = [fwd_b(s)[2] for s in sets]
    idx = {id(s): k for k, s in enumerate(sets)}
    fns_f = {"A": lambda s: fwd_a(s), "B": lambda s: fwd_b(s)}
    fns_b = {"A": lambda s: bwd_a(s, saved_a[idx[id(s)]]), "B": lambda s: bwd_b(s, saved_b[idx[id(s)]])}
    by = bytes_moved(B, T, R, H)
    print("(B, T, R, H) = %s, %d rotating buffer sets of %.0f MB, %d calls after %d warm-up:" % (
        (B, T, R, H), n_sets, one / 1e6, args.iters, args.warmup))
    for phase, fns in (("fwd", fns_f), ("bwd", fns_b)):
        res = alternate(fns, sets, args.warmup, args.iters)
        med = {k: statistics.median(v) for k, v in res.items()}
        for k in ("A", "B"):
            mb = by["%s %s" % (phase, k)] / 1e6
            print("  %s %s  median %8.1f us  (%s)   %7.1f MB to move -> %6.0f GB/s" % (
                phase, k, med[k], "  ".join("%.1f" % x for x in res[k]), mb, mb / med[k] * 1e3))
        print("  %s A / B = %.2f (time), %.2f (bytes)" % (phase, med["A"] / med["B"], by[phase + " A"] / by[phase + " B"]))


def whole_step(args):
    """Absolute time of a native BaseBertForVLTasks training step (no comparison partner on a GPU machine)."""
    import json
    import types
    from vilbert.basebert import BaseBertForVLTasks
    from vilbert.optim import AdamW
    cfg = json.load(open(os.path.join(ROOT, "vilbert-multi-task_amd", "config", "bert_base_baseline.json")))
    B, T, R = 128, 38, 101
    torch.manual_seed(0)
    net = BaseBertForVLTasks(types.SimpleNamespace(**cfg), num_labels=3129).to(DEV).train()
    net.set_active_heads(["vil_prediction"])
    optim = AdamW(net.parameters(), lr=4e-5)
    g = torch.Generator().manual_seed(3)
    inp = [torch.randint(0, cfg["vocab_size"], (B, T), generator=g).to(DEV), torch.rand(B, R, 2048, generator=g).to(DEV),
           torch.rand(B, R, 5, generator=g).to(DEV), torch.zeros(B, T, dtype=torch.long, device=DEV),
           torch.ones(B, T, dtype=torch.long, device=DEV), torch.ones(B, R, dtype=torch.long, device=DEV)]

    def step(_):
        optim.zero_grad(set_to_none=True)
        net(*inp)[0].square().mean().backward()
        optim.step()
    res = [timed(step, [None], 3, 10) / 1e3 for _ in range(REPEATS)]
    print("BaseBertForVLTasks step (bert_base_baseline, 12 layers, batch %d / %d tokens / %d regions, vil_prediction only, "
          "forward + backward + AdamW, dropout on): median %.1f ms  (%s)" % (B, T, R, statistics.median(res),
                                                                            "  ".join("%.1f" % x for x in res)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="also time a whole native BaseBertForVLTasks training step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("joint_embed_bench needs a GPU - nothing is measured without one")
    for shape in SHAPES:
        bench_shape(*shape, args)
    if args.step:
        whole_step(args)


if __name__ == "__main__":
    main()
