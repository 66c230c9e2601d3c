"""Golden trajectory of the reference's own RAdam and PlainRAdam (vilbert/optimization.py of the reference checkout) for
tests/test_radam.py and tests/test_radam_gpu.py. Only recorded NUMBERS are stored: the classes are imported from the
read-only reference checkout through oracle/ref_loader.py (package alias `vilbert_reference`) and run on the CPU as they
are - the installed torch still accepts their `add_(scalar, tensor)` call forms (with a deprecation warning).

The case (tests/radam_restatement.py: GOLDEN_*): 12 steps with beta2 = 0.999, so that the switch from the momentum step to
the rectified step falls at step 6; three small tensors in two groups (lr 1e-3 with weight decay 0.01 | lr 1e-5 without);
tensor 1 gets no gradient at steps 4 and 9 and falls behind; the learning rates shrink 5 % of their base value per step, so
that RAdam's step-size cache visibly hands a lagging tensor a step size computed under an older learning rate.

Stored: final parameters, both moments and step counts of both classes, RAdam's `buffer` after every step ([step, slot,
(step count, N_sma, step_size)], NaN = empty), and a `meta` JSON string.

Run in the build container:  python tests/golden/make_radam_golden.py   -> tests/golden/radam_trajectory.npz
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
import radam_restatement as rr  # noqa: E402
from oracle import ref_loader  # noqa: E402


def run_reference(cls):
    p0, grads = rr.golden_inputs()
    params = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = cls([{"params": [params[i] for i in g["idx"]], "lr": g["lr"], "weight_decay": g["weight_decay"]}
               for g in rr.GOLDEN_GROUPS])
    base = [g["lr"] for g in opt.param_groups]
    buffers = []
    for k, row in enumerate(grads):
        for g, lr in zip(opt.param_groups, base):
            g["lr"] = lr * rr.golden_lr_factor(k + 1)
        for p, t in zip(params, row):
            p.grad = None if t is None else t.clone()
        opt.step()
        if hasattr(opt, "buffer"):
            buffers.append([[np.nan if x is None else float(x) for x in slot] for slot in opt.buffer])
    out = {}
    for i, p in enumerate(params):
        out["p%d" % i] = p.detach().numpy().copy()
        out["m%d" % i] = opt.state[p]["exp_avg"].numpy().copy()
        out["v%d" % i] = opt.state[p]["exp_avg_sq"].numpy().copy()
    out["steps"] = np.array([opt.state[p]["step"] for p in params], dtype=np.int64)
    if buffers:
        out["buffer"] = np.array(buffers, dtype=np.float64)
    return out, opt


def main():
    ref_loader.load()
    ref = importlib.import_module("vilbert_reference.optimization")
    out = {}
    for name, cls in (("radam", ref.RAdam), ("plain", ref.PlainRAdam)):
        got, opt = run_reference(cls)
        out.update({"%s_%s" % (name, k): v for k, v in got.items()})
        keys = sorted(opt.state_dict()["state"][0])
    out["meta"] = np.array(json.dumps({
        "source": "the reference's own vilbert.optimization.RAdam / PlainRAdam, fp32 on the CPU, torch %s" % torch.__version__,
        "steps": rr.GOLDEN_STEPS, "sizes": list(rr.GOLDEN_SIZES), "groups": [dict(g) for g in rr.GOLDEN_GROUPS],
        "missing": sorted(rr.GOLDEN_MISSING), "lr_factor": "1 - 0.05 (step - 1)", "betas": [0.9, 0.999], "eps": 1e-8,
        "state_keys": keys}))
    np.savez_compressed(os.path.join(HERE, "radam_trajectory.npz"), **out)
    print({k: getattr(v, "shape", None) for k, v in out.items()})
    print(out["meta"])


if __name__ == "__main__":
    main()
