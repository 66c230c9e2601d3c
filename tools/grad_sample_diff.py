"""Compare two `bench.py --dump-outputs` directories of the pre-training step parameter by parameter.

gradients_sample / parameters_after_step_sample are bench.parameter_samples(): named_parameters() order, min(4096, numel)
elements each, so offset -> name needs only the model's parameter shapes (built on the CPU here, no GPU).

    python tools/grad_sample_diff.py PARENT_DIR BRANCH_DIR [--allow REGEX] [--config NAME.json]

Prints every parameter whose sampled gradient differs (max |diff|, relative to the tensor's sampled max), and checks:
  * the three losses are equal bit for bit;
  * outside --allow every sampled gradient is equal bit for bit;
  * inside --allow every one is within 2e-5 x max|parent| + 1e-6 x global max (tests/test_last_layer_rows_gpu.py::_close).
The default --allow names the output + feed-forward blocks of the last text and image layer, whose reductions over rows run on
the compact rows (csrc/layers.hip ffn_block_rows_bwd). Exit status 1 when a check fails."""
import argparse
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT]

BLOCK = r"(output\.dense|intermediate\.dense|attention\.output\.dense|attention\.output\.LayerNorm|output\.LayerNorm)\.(weight|bias)$"


def default_allow(cfg):
    lt, lv = cfg["num_hidden_layers"] - 1, cfg["v_num_hidden_layers"] - 1
    return r"encoder\.(layer\.%d|v_layer\.%d)\.%s" % (lt, lv, BLOCK)


def main():
    import bench
    import torch
    from vilbert.vilbert import BertConfig
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("branch")
    ap.add_argument("--allow", default=None)
    ap.add_argument("--config", default=bench.CONFIG)
    args = ap.parse_args()
    cfg = BertConfig.from_json_file(os.path.join(ROOT, "vilbert-multi-task_amd", "config", args.config)).to_dict()
    allow = re.compile(args.allow or default_allow(cfg))
    with torch.device("meta"):
        model = bench.build_model(cfg, "pretraining", "meta")
    names = [(n, min(4096, p.numel())) for n, p in model.named_parameters()]

    ok = True
    for loss in ("masked_lm_loss", "masked_img_loss", "next_sentence_loss"):
        a, b = (np.load(os.path.join(d, loss + ".npy")) for d in (args.parent, args.branch))
        same = a.tobytes() == b.tobytes()
        ok &= same
        print("%-20s parent %r branch %r %s" % (loss, a.reshape(-1)[:1].tolist(), b.reshape(-1)[:1].tolist(),
                                                "equal" if same else "DIFFERENT"))
    a, b = (np.load(os.path.join(d, "gradients_sample.npy")) for d in (args.parent, args.branch))
    assert a.shape == b.shape == (sum(k for _n, k in names),), (a.shape, b.shape, sum(k for _n, k in names))
    gmax = float(np.abs(a).max())
    off, worst, n_allowed, n_diff = 0, (0.0, None), 0, 0
    for name, k in names:
        pa, pb = a[off:off + k], b[off:off + k]
        off += k
        allowed = allow.search(name) is not None
        n_allowed += allowed
        if pa.tobytes() == pb.tobytes():
            continue
        n_diff += 1
        err, mx = float(np.abs(pa - pb).max()), float(np.abs(pa).max())
        rel = err / mx if mx > 0 else float("inf")
        good = allowed and err <= 2e-5 * mx + 1e-6 * gmax
        ok &= good
        if rel > worst[0]:
            worst = (rel, name)
        print("%-70s max|diff| %.3e  max %.3e  rel %.2e  %s" % (name, err, mx, rel, "ok" if good else (
            "OUT OF BOUND" if allowed else "NOT ALLOWED TO DIFFER")))
    print("%d parameters, %d allowed to differ, %d differ; global max %.3e; largest relative difference %.2e (%s)"
          % (len(names), n_allowed, n_diff, gmax, worst[0], worst[1]))
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
