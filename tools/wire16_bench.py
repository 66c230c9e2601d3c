"""What the half-width (float16) feature wire costs and saves (csrc/feat_rows.h, batch.hip, task_batch.hip; include/vilbert_hip_wire.h), against the fp32 path
at the same shapes in the same process:

  kernels   device events around back-to-back launches through the C ABI into preallocated outputs, per shape three legs that
            ALTERNATE inside every repeat: the fp32 call, the float16 call with fp32 output, the float16 call with bf16 output.
              concap   256 x 36 x 2048 (the pre-training batch): vb_concap_finish_batch / vbw_concap_finish_batch
              task     128 samples x 101 regions x 2048, 10 .. 100 packed rows per sample: vbd_task_finish_batch /
                       vbw_task_finish_batch
            Each leg rotates through SETS copies of its feature input and output (more than the 256 MiB last-level cache holds),
            so the GB/s are figures for memory traffic. The time of a call includes its small box / mask / label kernel, the
            same kernel in all three legs. The outputs are compared bit for bit before anything is timed.
  step      the pipeline-inclusive bf16 training step (bert_base_6layer_6conect, batch 256, 36 tokens, 36 + 1 regions, AdamW):
            numpy batches on the host each step -> DeviceBatchPipeline -> forward, backward, optimizer. Two legs that alternate
            inside every repeat: fp32 wire (the default pipeline) and float16 wire with bf16 feature output. Wall clock around
            whole runs that end in a device synchronise. The leg is host-bound; read the spread before the difference.

Every leg is warmed up, then timed REPEATS times; median and range are printed. The spread of the fp32 leg is the margin: a
difference inside it is not a difference.

The driver (no --leg) touches no device: it starts each leg as a fresh child process under its own time limit, stops at the first
failure and writes what the legs printed to profiles/wire16_ab.txt.

    python tools/wire16_bench.py [--iters 200] [--warmup 20] [--steps 8] [--out profiles/wire16_ab.txt]
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
REPEATS = 5
SETS = 6          # buffer sets a kernel leg rotates through: at least 450 MB per leg
F = 2048
CONCAP = dict(B=256, R=36, T=36)
TASK = dict(B=128, R=101)
LEG_LIMITS = {"kernels": 300, "step": 400}          # seconds, per child process


def event_leg(fn, warmup, iters):
    import torch
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


def show(name, values, unit, nbytes=None):
    med = statistics.median(values)
    tail = "" if nbytes is None else "   %6.1f MB -> %5.0f GB/s" % (nbytes / 1e6, nbytes / 1e6 / med)
    print("  %-34s median %9.4f %s   (range %.4f .. %.4f over %d repeats)%s"
          % (name, med, unit, min(values), max(values), len(values), tail))
    return med


def verdict(name, base, new):
    """The margin is the run-to-run spread of the fp32 leg in this very run."""
    spread = max(base) - min(base)
    diff = statistics.median(new) - statistics.median(base)
    word = "inside the fp32 leg's spread" if abs(diff) <= spread else ("FASTER" if diff < 0 else "SLOWER")
    print("      %s vs fp32: %+.4f ms (%+.1f %%), fp32 spread %.4f ms: %s"
          % (name, diff, 100.0 * diff / statistics.median(base), spread, word))


def half_values(shape, seed):
    """Post-ReLU-like float16 features: non-negative, full mantissas."""
    g = np.random.RandomState(seed)
    return (g.rand(*shape).astype(np.float32) * 2).astype(np.float16)


# ---- kernels -------------------------------------------------------------------------------------------------------------------
def concap_legs():
    import torch
    from vilbert import _native as N
    lib = N.lib()
    B, R, T = CONCAP["B"], CONCAP["R"], CONCAP["T"]
    g = torch.Generator().manual_seed(1)
    half = torch.from_numpy(half_values((B, R, F), 1)).to(DEV)
    small = dict(image_loc=torch.rand(B, R, 5, generator=g).to(DEV), image_mask=torch.ones(B, R, dtype=torch.int64, device=DEV),
                 masked_label=(torch.rand(B, R, generator=g) < 0.2).long().to(DEV),
                 is_next=torch.zeros(B, dtype=torch.int64, device=DEV), image_label=torch.zeros(B, R, dtype=torch.int64, device=DEV),
                 lm_label_ids=torch.zeros(B, T, dtype=torch.int64, device=DEV),
                 out_image_loc=torch.empty(B, R + 1, 5, device=DEV), out_image_mask=torch.empty(B, R + 1, dtype=torch.int64, device=DEV),
                 out_image_label=torch.empty(B, R, dtype=torch.int64, device=DEV),
                 out_lm_label_ids=torch.empty(B, T, dtype=torch.int64, device=DEV))
    keep, legs = [half, small], {}
    for name, in_dt, out_dt, kind in (("fp32", torch.float32, torch.float32, None), ("f16 -> fp32", torch.float16, torch.float32, 0),
                                      ("f16 -> bf16", torch.float16, torch.bfloat16, 1)):
        sets = []
        for _ in range(SETS):
            a = N.ConcapBatch() if kind is None else N.WireConcapBatch()
            a.batch, a.regions, a.tokens, a.feat_dim, a.objective = B, R, T, F, 0
            if kind is not None:
                a.out_kind = kind
            big = dict(image_feat=half.to(in_dt, copy=True), out_image_feat=torch.empty(B, R + 1, F, dtype=out_dt, device=DEV))
            for k, t in list(small.items()) + list(big.items()):
                setattr(a, k, t.data_ptr())
            sets.append((a, big))
        call = lib.vb_concap_finish_batch if kind is None else lib.vbw_concap_finish_batch
        nbytes = B * F * (R * sets[0][1]["image_feat"].element_size() + (R + 1) * sets[0][1]["out_image_feat"].element_size())
        turn = [0]

        def fn(sets=sets, call=call, turn=turn, what=name):
            turn[0] = (turn[0] + 1) % SETS
            N.check(call(N.stream_ptr(), ctypes.byref(sets[turn[0]][0])), what)
        legs[name] = (fn, nbytes, sets)
        keep.append(sets)
    return legs, keep, "out_image_feat"


def task_legs():
    import torch
    import task_batch_restatement as tr
    from vilbert import _native as N
    from vilbert import task_pipeline as tp
    lib = N.lib()
    B, R = TASK["B"], TASK["R"]
    rng = np.random.default_rng(1)
    packed = tr.make_packed(rng.integers(10, 101, B).tolist(), F, seed=1)
    n = packed["feat"].shape[0]
    half = torch.from_numpy(half_values((n, F), 2)).to(DEV)
    fields = ("boxes", "offsets", "image_wh")               # mean_rows stays NULL: every row of a sample enters its mean
    assert set(fields) < set(tp.PACKED_FIELDS)
    dev = {k: torch.from_numpy(np.ascontiguousarray(packed[k])).to(DEV) for k in fields}
    outs = [torch.empty(B, R, 5, device=DEV), torch.empty(B, R, dtype=torch.int64, device=DEV)]
    keep, legs = [half, dev, outs], {}
    for name, in_dt, out_dt, kind in (("fp32", torch.float32, torch.float32, None), ("f16 -> fp32", torch.float16, torch.float32, 0),
                                      ("f16 -> bf16", torch.float16, torch.bfloat16, 1)):
        sets = []
        for _ in range(SETS):
            a = N.TaskBatchArgs() if kind is None else N.WireTaskBatch()
            a.batch, a.max_regions, a.feat_dim, a.iou_floor, a.total_rows = B, R, F, 0.0, n
            if kind is not None:
                a.out_kind = kind
            big = dict(feat=half.to(in_dt, copy=True), out_feat=torch.empty(B, R, F, dtype=out_dt, device=DEV))
            a.feat, a.out_feat = big["feat"].data_ptr(), big["out_feat"].data_ptr()
            a.boxes, a.offsets, a.image_wh = (dev[k].data_ptr() for k in fields)
            a.out_spatials, a.out_mask = outs[0].data_ptr(), outs[1].data_ptr()
            sets.append((a, big))
        call = lib.vbd_task_finish_batch if kind is None else lib.vbw_task_finish_batch
        nbytes = F * (n * sets[0][1]["feat"].element_size() + B * R * sets[0][1]["out_feat"].element_size())
        turn = [0]

        def fn(sets=sets, call=call, turn=turn, what=name):
            turn[0] = (turn[0] + 1) % SETS
            N.check(call(N.stream_ptr(), ctypes.byref(sets[turn[0]][0])), what)
        legs[name] = (fn, nbytes, sets)
        keep.append(sets)
    return legs, keep, "out_feat", n


def check_legs(legs, out_name):
    """fp32 leg = yardstick: the float16 legs give its bits, or its bits rounded to bf16 (every set is written once first)."""
    import torch
    for fn, _, _ in legs.values():
        for _ in range(SETS):
            fn()
    torch.cuda.synchronize()
    want = legs["fp32"][2][0][1][out_name]
    for name, (_, _, sets) in legs.items():
        for _, big in sets:
            got = big[out_name]
            assert torch.equal(got, want if got.dtype == torch.float32 else want.to(torch.bfloat16)), name


def run_kernels(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("wire16_bench needs a GPU - nothing is measured without one")
    print("feature kernels, device events around %d back-to-back calls per repeat, legs alternating, %d buffer sets per leg; "
          "outputs agree bit for bit with the fp32 call (bf16: its rounding)" % (args.iters, SETS))
    for title, built in (("concap  %(B)d x %(R)d x 2048" % CONCAP, concap_legs()), ("task    %(B)d samples x %(R)d regions x 2048" % TASK, task_legs())):
        legs, keep, out_name = built[:3]
        check_legs(legs, out_name)
        print(title + ("" if len(built) == 3 else ", %d packed rows" % built[3]))
        res = {name: [] for name in legs}
        for _ in range(REPEATS):
            for name, (fn, _, _) in legs.items():
                res[name].append(event_leg(fn, args.warmup, args.iters))
        for name, (_, nbytes, _) in legs.items():
            show(name, res[name], "ms per call", nbytes)
        for name in ("f16 -> fp32", "f16 -> bf16"):
            verdict(name, res["fp32"], res[name])
        del legs, keep, built
        torch.cuda.empty_cache()


# ---- the pipeline-inclusive step -----------------------------------------------------------------------------------------------
def run_step(args):
    import json
    import torch
    from vilbert.input_pipeline import DeviceBatchPipeline
    from vilbert.optim import AdamW
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    if not torch.cuda.is_available():
        raise SystemExit("wire16_bench needs a GPU - nothing is measured without one")
    cfg = json.load(open(os.path.join(ROOT, "vilbert-multi-task_amd", "config", "bert_base_6layer_6conect.json")))
    B, T, R = CONCAP["B"], CONCAP["T"], CONCAP["R"]
    torch.manual_seed(1234)
    model = BertForMultiModalPreTraining(BertConfig.from_dict(cfg)).to(DEV).train().half()
    opt = AdamW(model.parameters(), lr=1e-4, betas=(0.9, 0.98))
    g = np.random.RandomState(5)
    wires = {"fp32 wire": [], "f16 wire, bf16 features": []}
    for i in range(2):
        ids = g.randint(0, cfg["vocab_size"], size=(B, T)).astype(np.int64)
        lm = np.where(g.rand(B, T) < 0.15, ids, -1).astype(np.int64)
        lm[:, 1] = ids[:, 1]
        il = np.where(g.rand(B, R) < 0.15, 1, -1).astype(np.int64)
        il[:, 0] = 1
        tgt = g.rand(B, R, cfg["v_target_size"]).astype(np.float32)
        tgt = (tgt / tgt.sum(-1, keepdims=True)).astype(np.float16)
        feat = half_values((B, R, cfg["v_feature_size"]), 10 + i)
        rest = (ids, np.ones((B, T), np.int64), np.zeros((B, T), np.int64), lm, np.zeros(B, np.int64))
        tail = (il, np.ones((B, R), np.int64), (il == 1).astype(np.int64))
        loc = g.rand(B, R, 5).astype(np.float32)
        wires["f16 wire, bf16 features"].append(rest + (feat, loc, tgt) + tail)
        wires["fp32 wire"].append(rest + (feat.astype(np.float32), loc, tgt.astype(np.float32)) + tail)
    kwargs = {"fp32 wire": {}, "f16 wire, bf16 features": dict(wire_dtype=torch.float16, feature_dtype=torch.bfloat16)}

    def run(name, n):
        raws = wires[name]
        t0 = time.perf_counter()
        for b in DeviceBatchPipeline((raws[i % 2] for i in range(n)), DEV, objective=1, **kwargs[name]):
            input_ids, input_mask, segment_ids, lm_label_ids, is_next, feat, loc, target, ilabel, imask = b
            opt.zero_grad(set_to_none=True)
            lm_l, img_l, nsp_l = model(input_ids, feat, loc, segment_ids, input_mask, imask, lm_label_ids, ilabel, target, is_next)
            (lm_l.mean() + img_l.mean() + nsp_l.mean()).backward()
            opt.step()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / n

    for name in wires:
        run(name, 3)
    res = {name: [] for name in wires}
    for _ in range(REPEATS):
        for name in wires:
            res[name].append(run(name, args.steps))
    mb = {name: sum(a.nbytes for a in raws[0]) / 1e6 for name, raws in wires.items()}
    print("pipeline-inclusive bf16 training step, bert_base_6layer_6conect, batch %d, %d tokens, %d + 1 regions: numpy batches on the "
          "host -> DeviceBatchPipeline -> forward, backward, AdamW; wall clock over %d steps per repeat, legs alternating" % (B, T, R, args.steps))
    for name in wires:
        show("%s (%.1f MB per step)" % (name, mb[name]), res[name], "ms per step")
    verdict("f16 wire", res["fp32 wire"], res["f16 wire, bf16 features"])
    print("      (host-bound leg: machines differ by up to 30 %; only a difference beyond the spread above is one)")


# ---- the driver ----------------------------------------------------------------------------------------------------------------
def drive(args):
    """Each leg in a fresh child process under its own time limit; stop at the first failure."""
    lines = []
    for leg in ("kernels", "step"):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--iters", str(args.iters), "--warmup", str(args.warmup),
               "--steps", str(args.steps)]
        print("# leg %s (limit %d s)" % (leg, LEG_LIMITS[leg]))
        sys.stdout.flush()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LEG_LIMITS[leg])
        except subprocess.TimeoutExpired:
            print("leg %s exceeded its limit of %d s - stopping" % (leg, LEG_LIMITS[leg]))
            return 124
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr[-4000:])
            print("leg %s failed with exit status %d - stopping" % (leg, r.returncode))
            return r.returncode or 1
        lines.append(r.stdout)
    out = os.path.join(ROOT, args.out)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("".join(lines))
    print("written to %s" % args.out)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=8, help="training steps per timed run of the step leg")
    ap.add_argument("--out", default=os.path.join("profiles", "wire16_ab.txt"), help="relative to the repository root")
    ap.add_argument("--leg", choices=["kernels", "step"], default=None, help="run one leg in this process (the driver does)")
    args = ap.parse_args()
    if args.leg is None:
        sys.exit(drive(args))
    {"kernels": run_kernels, "step": run_step}[args.leg](args)


if __name__ == "__main__":
    main()
