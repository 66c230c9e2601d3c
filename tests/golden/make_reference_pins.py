"""Generate tests/golden/reference_pins.{json,npz} from the REAL reference (a machine with the reference tree only).

    VILBERT_REFERENCE_ROOT=/path/to/vilbert-multi-task python tests/golden/make_reference_pins.py

What the CPU tests compare the package and the oracle with, recorded from the reference so that the tests run
without it: the state_dict / named_parameters / named_modules tables, BertConfig defaults and the shipped config
files, constructor / forward signatures, forward outputs, pre-training losses and gradients, and - as sha256
digests of dtype, shape and bytes, for the bit-exact comparisons - the reference loader's batch finishing and
ForwardModelsTrain's model arguments and loss. Float arrays are kept as strided samples of at most OUTPUT_CAP
(GRADIENT_CAP for gradients) elements each, with their shape and largest |value|; the tests that compare with them
also compare every element against the reference itself where its tree is present (reference_vltasks,
reference_pretraining). Nothing of the reference is copied; only values derived by running it.
"""
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "vilbert-multi-task_amd")
for p in (HERE, TESTS, PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import cases  # noqa: E402
from oracle import batch_oracle as bo, ref_loader, synth  # noqa: E402

# the parametrisations of the tests that read the pins
STATE_DICT_CFGS = ["tiny", "tiny_task", "bert_base_2layer_2conect.json"]
SIGNATURE_CLASSES = ["BertConfig", "BertEmbeddings", "BertImageEmbeddings", "BertSelfAttention", "BertSelfOutput",
                     "BertAttention", "BertIntermediate", "BertOutput", "BertLayer", "BertImageSelfAttention",
                     "BertImageSelfOutput", "BertImageAttention", "BertImageIntermediate", "BertImageOutput",
                     "BertImageLayer", "BertBiAttention", "BertBiOutput", "BertConnectionLayer", "BertEncoder",
                     "BertTextPooler", "BertImagePooler", "BertModel", "BertPreTrainingHeads",
                     "BertForMultiModalPreTraining", "VILBertForVLTasks", "SimpleClassifier"]
PIPELINE_CASES = [(3, dict(batch=5, tokens=12, regions=9, feat_dim=32, n_classes=7)),
                  (4, dict(batch=3, tokens=36, regions=36, feat_dim=2048, n_classes=1601))]
PRETRAINING_TARGET_SEED = 17
OUTPUT_CAP, GRADIENT_CAP = 256, 128


def _cap(key):
    return GRADIENT_CAP if "/grad/" in key else OUTPUT_CAP


def state_dict_cfg(name):
    if name == "tiny":
        return synth.tiny_config()
    if name == "tiny_task":
        return synth.tiny_config(task_specific_tokens=True)
    return dict(synth.load_config(name), num_hidden_layers=2, t_biattention_id=[0, 1])  # keep the ctor cheap


def pretraining_case(visual_target):
    """(cfg, state dict, positional args) of the pre-training losses / gradients comparison."""
    cfg = synth.tiny_config(visual_target=visual_target, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
                            v_hidden_dropout_prob=0.0, v_attention_probs_dropout_prob=0.0)
    sd = synth.make_state_dict(cfg, "pretraining")
    x = synth.make_inputs(cfg, 4, 9, 8, with_labels=True)
    if visual_target == 1:
        g = torch.Generator().manual_seed(PRETRAINING_TARGET_SEED)
        x["image_target"] = torch.randn(4, 7, cfg["v_target_size"], generator=g)
    args = tuple(x[n] for n in ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask",
                                "image_attention_mask", "masked_lm_labels", "image_label", "image_target",
                                "next_sentence_label"))
    return cfg, sd, args


def vltasks_case():
    cfg = synth.tiny_config()
    return cfg, synth.make_state_dict(cfg, "vltasks"), vltasks_args(synth.make_inputs(cfg, 4, 9, 7))


def task_tokens_case():
    cfg = synth.tiny_config(task_specific_tokens=True)
    return cfg, synth.make_state_dict(cfg, "vltasks"), vltasks_args(synth.make_inputs(cfg, 3, 6, 5, task_id=4))


def vltasks_args(x):
    args = [x[n] for n in ("input_ids", "image_feat", "image_loc", "token_type_ids", "attention_mask",
                           "image_attention_mask", "co_attention_mask")]
    if "task_ids" in x:
        args.append(x["task_ids"])
    return tuple(args)


def reference_vltasks(cfg, sd, args):
    """The reference VILBertForVLTasks's first nine outputs (eval, no_grad)."""
    ref = ref_loader.load()
    m = ref.VILBertForVLTasks(ref.BertConfig.from_dict(cfg), num_labels=1)
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    with torch.no_grad():
        return m.eval()(*args)[:9]


def reference_pretraining(cfg, sd, args):
    """(losses, {parameter name: gradient or None}) of the reference pre-training wrapper, dropout off."""
    ref = ref_loader.load()
    m = ref.BertForMultiModalPreTraining(ref.BertConfig.from_dict(cfg))
    res = m.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    m.cls.dropout.p = 0.0
    m.train()
    losses = m(*args)
    sum(l.sum() for l in losses).backward()
    return [l.detach() for l in losses], {n: p.grad for n, p in m.named_parameters()}


def _json_lines(key, value):
    dump = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))
    if not isinstance(value, dict) or not value:
        return "%s:%s" % (dump(key), dump(value))
    return "%s:{\n%s\n}" % (dump(key), ",\n".join("%s:%s" % (dump(k), dump(value[k])) for k in sorted(value)))


def config_digest(d):
    return hashlib.sha256(json.dumps(d, sort_keys=True).encode()).hexdigest()


def main():
    import inspect
    ref = ref_loader.load()
    pins, arrays = {}, {}

    def ref_model(cfg, kind, sd=None):
        rc = ref.BertConfig.from_dict(cfg)
        m = ref.BertForMultiModalPreTraining(rc) if kind == "pretraining" else ref.VILBertForVLTasks(rc, num_labels=1)
        if sd is not None:
            res = m.load_state_dict(sd, strict=True)
            assert not res.missing_keys and not res.unexpected_keys
        return m

    # state_dict order / shapes (tests/test_oracle_vs_reference.py)
    pins["state_dict"] = {}
    for kind in ("pretraining", "vltasks"):
        for name in STATE_DICT_CFGS:
            m = ref_model(state_dict_cfg(name), kind)
            pins["state_dict"]["%s/%s" % (kind, name)] = [[k, list(v.shape)] for k, v in m.state_dict().items()]

    # forward outputs of the tiny model, with and without task tokens
    for tag, (cfg, sd, args) in (("vltasks_forward", vltasks_case()), ("task_tokens", task_tokens_case())):
        for i, o in enumerate(reference_vltasks(cfg, sd, args)):
            arrays["%s/%d" % (tag, i)] = o.numpy()

    # pre-training losses and parameter gradients (dropout off)
    for vt in (0, 1):
        losses, grads = reference_pretraining(*pretraining_case(vt))
        for i, l in enumerate(losses):
            arrays["pretraining_vt%d/loss/%d" % (vt, i)] = l.numpy()
        pins["pretraining_vt%d_no_grad" % vt] = [n for n, g in grads.items() if g is None]
        for name, g in grads.items():
            if g is not None:
                arrays["pretraining_vt%d/grad/%s" % (vt, name)] = g.numpy()

    # boundary (tests/test_boundary.py)
    cfg = synth.tiny_config(task_specific_tokens=True)
    m = ref.VILBertForVLTasks(ref.BertConfig.from_dict(cfg), 1)
    pins["named_parameters"] = [[n, list(p.shape)] for n, p in m.named_parameters()]
    pins["named_modules"] = [n for n, _ in m.named_modules()]
    pins["config_defaults"] = ref.BertConfig(123).to_dict()
    pins["config_from_json"] = {
        name: ref.BertConfig.from_json_file(ref_loader.config_path(name)).to_dict()
        for name in sorted(os.listdir(synth.CONFIG_DIR)) if name.endswith(".json") and "6conect" in name}
    sigs = {}
    for name in SIGNATURE_CLASSES:
        theirs = getattr(ref, name, None)
        if theirs is None:
            continue
        for meth in ("__init__", "forward"):
            if not hasattr(theirs, meth) or getattr(theirs, meth) is getattr(object, meth, None):
                continue
            sigs["%s.%s" % (name, meth)] = cases.signature_rows(getattr(theirs, meth))
    pins["signatures"] = sigs
    pins["config_method_signatures"] = {fn: str(inspect.signature(getattr(ref.BertConfig, fn)))
                                        for fn in ("from_dict", "from_json_file", "to_dict", "to_json_string")}

    # encoder schedules of every shipped config (tests/test_encoder_schedules.py)
    import test_encoder_schedules as tes
    pins["config_file_sha256"] = {}
    for cfgname in tes.SHIPPED:
        pins["config_file_sha256"][cfgname] = config_digest(json.load(open(ref_loader.config_path(cfgname))))
        for i, o in enumerate(reference_vltasks(*tes.schedule_case(cfgname))):
            arrays["schedule/%s/%d" % (cfgname, i)] = o.numpy()

    # the reference loader's batch finishing, bit-exact (tests/test_input_pipeline.py)
    import ref_loader_source as rls
    pins["batch_finishing"] = {}
    for seed, shape in PIPELINE_CASES:
        raw = bo.make_raw_batch(seed=seed, **shape)
        tup = tuple(raw[n].copy() for n in bo.RAW_FIELDS) + (np.arange(shape["batch"]),)
        got = rls.reference_loader_iter([tup])[0]
        il1, lm1 = rls.reference_objective1_edit(torch.tensor(raw["image_label"]), torch.tensor(raw["lm_label_ids"]),
                                                 torch.tensor(raw["is_next"]))
        pins["batch_finishing"][str(seed)] = {"objective0": [cases.digest(got[i]) for i in range(len(bo.OUT_FIELDS))],
                                              "image_label": cases.digest(il1), "lm_label_ids": cases.digest(lm1)}

    # ForwardModelsTrain on a canned model, bit-exact (tests/test_reference_scripts.py); last: it attaches the reference
    # to the product package
    import yaml
    import vilbert
    from oracle import task_forward_oracle as tf
    from test_reference_scripts import _CannedModel, _Loader
    vilbert.attach_reference(ref_loader.REFERENCE_ROOT)
    from vilbert import _compat
    _compat.install()
    if ref_loader.REFERENCE_ROOT not in sys.path:
        sys.path.append(ref_loader.REFERENCE_ROOT)
    import vilbert.task_utils as TU
    torch.Tensor.cuda = lambda self, *a, **k: self
    task_cfg = yaml.safe_load(open(os.path.join(ref_loader.REFERENCE_ROOT, "vilbert_tasks.yml")))
    pins["forward_models_train"] = {}
    for task_id in sorted(tf.TASKS):
        kind, _, _ = tf.TASKS[task_id]
        batch = tf.make_task_batch(task_id, 4, 7, 110 if kind == "V-logit-mc" else 9, seed=5)
        model = _CannedModel(3129, 3)
        losses = TU.LoadLosses(None, task_cfg, [task_id[4:]])
        loss, score = TU.ForwardModelsTrain(None, task_cfg, "cpu", task_id, {task_id: 0}, {task_id: None},
                                            {task_id: _Loader([batch])}, model, losses)
        pins["forward_models_train"][task_id] = {
            "type_loss_process": [task_cfg[task_id]["type"], task_cfg[task_id]["loss"], task_cfg[task_id]["process"]],
            "calls": len(model.calls), "model_args": [cases.digest(t) for t in model.calls[0]],
            "loss": cases.digest(loss.detach()), "score": float(score)}

    pins["arrays"], values = cases.pack_pins(arrays, _cap)
    with open(cases.PINS_JSON, "w") as f:      # one line per entry of the top two levels: small, and diffs stay readable
        f.write("{\n" + ",\n".join(_json_lines(k, pins[k]) for k in sorted(pins)) + "\n}\n")
    np.savez_compressed(cases.PINS_NPZ, values=values)
    print("wrote %s (%d keys) and %s (%d arrays, %d values)" % (cases.PINS_JSON, len(pins), cases.PINS_NPZ, len(arrays),
                                                             values.size))


if __name__ == "__main__":
    main()
