"""One eager pre-training step through every route to the three losses, dumped for a bit-for-bit comparison of two commits.

bert_base_2layer_2conect.json at B, T, R = 4, 36, 37 (the smallest shape that passes the bf16 eligibility rules), weights and
inputs of oracle/synth.py, torch.manual_seed fixed, dropout ON. One step for every combination of
    visual target 0 (KL), 1 (squared error), 2 (NCE)  x  GEMM mode f32, bf16  x  label_capacity None (exact gather), 0.5
- on the fp32 stream that is the full-row route and the last-layer row maps, on the bf16 stream the compact bf16 rows. All
twelve run in ONE process, in a fixed order: the dropout / NCE seeds are a per-process counter, so a seed drawn in another
place or order shows in every later combination too. Per combination one DIR/t<target>_<mode>_<gather>.npz with the three
losses and the gradient of every parameter. Needs a GPU.

    python tools/pretrain_routes_dump.py DIR              # dump
    python tools/pretrain_routes_dump.py DIR --against OTHER_DIR    # compare two dumps: tobytes() equality, exit status 1 if not
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "vilbert-multi-task_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
B, T, R = 4, 36, 37
NAMES = ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask", "image_attention_mask",
         "masked_lm_labels", "image_label", "image_target", "next_sentence_label")
LOSSES = ("masked_lm_loss", "masked_img_loss", "next_sentence_loss")
COMBINATIONS = [(target, mode, capacity) for target in (0, 1, 2) for mode in ("f32", "bf16") for capacity in (None, 0.5)]


def _file(outdir, target, mode, capacity):
    return os.path.join(outdir, "t%d_%s_%s.npz" % (target, mode, "exact" if capacity is None else "cap%g" % capacity))


def dump(outdir):
    from oracle import synth
    from vilbert import _native
    from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining
    os.makedirs(outdir, exist_ok=True)
    torch.manual_seed(1234)
    for target, mode, capacity in COMBINATIONS:
        cfg = synth.load_config("bert_base_2layer_2conect.json")
        cfg["visual_target"] = target
        if target != 0:
            cfg["v_target_size"] = cfg["v_feature_size"]      # targets 1 and 2 regress / contrast region FEATURES
        sd = synth.make_state_dict(cfg, "pretraining")
        x = synth.make_inputs(cfg, B, T, R, with_labels=True)
        if target != 0:
            x["image_target"] = torch.randn(x["image_target"].shape, generator=torch.Generator().manual_seed(8))
        model = BertForMultiModalPreTraining(BertConfig.from_dict(cfg))
        model.load_state_dict(sd)
        model = model.to(DEV).train()
        model.label_capacity = capacity
        prev = _native.set_gemm_mode(mode)
        try:
            losses = model(*[x[n].to(DEV) for n in NAMES])
            sum(l.sum() for l in losses).backward()
        finally:
            _native.set_gemm_mode(prev)
        torch.cuda.synchronize()
        if capacity is not None:
            model.check_label_capacity()
        arrays = {name: l.detach().cpu().numpy() for name, l in zip(LOSSES, losses)}
        arrays.update(("grad/" + n, p.grad.detach().cpu().numpy()) for n, p in model.named_parameters() if p.grad is not None)
        np.savez(_file(outdir, target, mode, capacity), **arrays)
        print("target %d  %-4s  label_capacity %-4s  losses %s  %d gradients" % (
            target, mode, capacity, " ".join("%.6f" % float(arrays[n].reshape(-1)[0]) for n in LOSSES), len(arrays) - 3),
            flush=True)
        del model, losses, arrays


def compare(a_dir, b_dir):
    ok = True
    for combination in COMBINATIONS:
        a, b = np.load(_file(a_dir, *combination)), np.load(_file(b_dir, *combination))
        differ = sorted(set(a.files) ^ set(b.files)) + [n for n in a.files if n in b.files and (
            a[n].dtype != b[n].dtype or a[n].shape != b[n].shape or a[n].tobytes() != b[n].tobytes())]
        ok &= not differ
        print("%-22s %d arrays: %s" % (os.path.basename(_file("", *combination)), len(a.files),
                                        "bit-equal" if not differ else "DIFFERENT: " + ", ".join(differ[:8])))
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--against", metavar="OTHER_DIR", default=None)
    args = ap.parse_args()
    sys.exit(compare(args.dir, args.against) if args.against else dump(args.dir))
