"""Records the fixtures of the single-stream baseline model from the REAL reference (vilbert/basebert.py of the reference
checkout, $VILBERT_REFERENCE_ROOT or oracle.ref_loader.REFERENCE_ROOT). Runs on the CPU, where a checkout exists; the tests
read only what it writes:

    tests/golden/basebert_state_dict.json   [name, shape] of BaseBertForVLTasks(tiny config, 13).state_dict(), in order
    tests/golden/basebert_tiny.npz          the seven outputs, and the parameter gradients of basebert_synth.weighted_loss as
                                            strided pins (cases.pack_pins) with each tensor's max |grad| and the exact rows 0
                                            of the four padding_idx tables
    tests/golden/basebert_base_2l.npz       the seven outputs of bert_base_baseline.json with two layers at B=2, T=38, R=101
                                            (strided on the two wide ones)

Everything is recorded in eval mode: in train mode the reference's own backward raises (the in-place dropout behind the ReLU
of its SimpleClassifier). Weights and inputs come from tests/basebert_synth.py.

    python tests/golden/make_basebert_golden.py
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import basebert_synth as BS  # noqa: E402
import cases  # noqa: E402
from oracle import ref_loader  # noqa: E402


def _load_file(alias, file_path):
    spec = importlib.util.spec_from_file_location(alias, file_path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[alias] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    """The reference's basebert module under an alias, with its three foreign imports satisfied: vilbert.utils is the
    reference's own utils.py, pytorch_transformers.modeling_bert.BertConfig an attribute bag, apex unimportable (so the
    reference's pure-Python BertLayerNorm is used)."""
    ref_dir = os.path.join(ref_loader.REFERENCE_ROOT, "vilbert")
    ref_loader._install_stubs()
    saved = {k: sys.modules.get(k) for k in ("vilbert", "vilbert.utils", "pytorch_transformers",
                                             "pytorch_transformers.modeling_bert", "apex")}
    utils = _load_file("vilbert_reference_utils", os.path.join(ref_dir, "utils.py"))
    pkg = types.ModuleType("vilbert")
    pkg.__path__ = []
    pkg.utils = utils
    pt, mb = types.ModuleType("pytorch_transformers"), types.ModuleType("pytorch_transformers.modeling_bert")

    class BertConfig(types.SimpleNamespace):
        pass

    mb.BertConfig, pt.modeling_bert = BertConfig, mb
    sys.modules.update({"vilbert": pkg, "vilbert.utils": utils, "pytorch_transformers": pt,
                        "pytorch_transformers.modeling_bert": mb, "apex": None})
    try:
        mod = _load_file("vilbert_reference_basebert", os.path.join(ref_dir, "basebert.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod, BertConfig


def build(ref, BertConfig, case):
    c = BS.CASES[case]
    torch.manual_seed(0)
    model = ref.BaseBertForVLTasks(BertConfig(**c["cfg"]()), num_labels=c["num_labels"])
    shapes = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    model.load_state_dict(BS.make_state_dict(shapes))
    return model.eval(), shapes


def main():
    ref, BertConfig = load_reference()

    # ---- case A: tiny model, outputs and gradients ----
    case = "basebert_tiny"
    model, shapes = build(ref, BertConfig, case)
    with open(BS.NAMES_JSON, "w") as f:
        json.dump([[k, list(s)] for k, s in shapes], f, indent=0)
        f.write("\n")
    x = BS.make_inputs(case)
    outs = model(*BS.forward_args(x))
    BS.weighted_loss(outs, x["image_attention_mask"]).backward()
    grads = {n: p.grad.numpy() for n, p in model.named_parameters() if p.grad is not None}
    index, values = cases.pack_pins(grads, lambda key: BS.PIN_CAP)
    store = {n: BS.sample(case, n, o.detach()).numpy() for n, o in zip(BS.HEADS, outs)}
    store["grad_values"] = values
    store["grad_index"] = np.array(json.dumps(index))
    for i, name in enumerate(BS.PADDED_TABLES):
        store["grad_row0_%d" % i] = grads[name][0].copy()
    np.savez_compressed(BS.path(case), **store)

    # ---- case B: the base model at the task shape, outputs ----
    case = "basebert_base_2l"
    model, _ = build(ref, BertConfig, case)
    x = BS.make_inputs(case)
    with torch.no_grad():
        outs = model(*BS.forward_args(x))
    np.savez_compressed(BS.path(case), **{n: BS.sample(case, n, o).numpy() for n, o in zip(BS.HEADS, outs)})
    for p in (BS.NAMES_JSON, BS.path("basebert_tiny"), BS.path("basebert_base_2l")):
        print("%8d bytes  %s" % (os.path.getsize(p), os.path.relpath(p)))
        assert os.path.getsize(p) < 500 * 1000, p


if __name__ == "__main__":
    main()
