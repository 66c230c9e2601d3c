"""Seeded weights, inputs and cases for the single-stream baseline model (vilbert/basebert.py). TEST INFRASTRUCTURE shared by
tests/golden/make_basebert_golden.py (which runs the real reference) and the tests: weights and inputs are regenerated from
per-tensor seeds, only the reference's outputs are committed."""
import os
import sys
import types
import zlib

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import synth  # noqa: E402

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES_JSON = os.path.join(GOLDEN_DIR, "basebert_state_dict.json")
HEADS = ["vil_prediction", "vil_logit", "vil_binary_prediction", "vision_prediction", "vision_logit", "linguisic_prediction",
         "linguisic_logit"]
# weights of loss = sum_i w_i * out_i (tests/test_backward_gpu.py::_grad_parity's, for the seven heads of this model); the
# vision_logit term is multiplied by the image mask instead (its -10000 entries are excluded)
LOSS_WEIGHTS = {"vil_prediction": 1.0, "vil_logit": 1.3, "vil_binary_prediction": 0.9, "vision_prediction": 0.01,
                "vision_logit": None, "linguisic_prediction": 0.002, "linguisic_logit": 1.0}
PADDED_TABLES = ["bert.embeddings.word_embeddings.weight", "bert.embeddings.position_embeddings.weight",
                 "bert.embeddings.token_type_embeddings.weight", "bert.image_embeddings.token_type_embeddings.weight"]
PIN_CAP = 600          # pinned gradient elements per tensor

TINY = dict(vocab_size=97, hidden_size=64, num_attention_heads=2, intermediate_size=128, max_position_embeddings=40,
            num_hidden_layers=2, type_vocab_size=2, hidden_act="gelu", hidden_dropout_prob=0.1,
            attention_probs_dropout_prob=0.1, initializer_range=0.02)

# name -> dict(cfg (callable), num_labels, batch, n_tok, n_reg, stride{output: step along the last dim})
CASES = {
    "basebert_tiny": dict(cfg=lambda: dict(TINY), num_labels=13, batch=3, n_tok=7, n_reg=5),
    "basebert_base_2l": dict(cfg=lambda: dict(_json("bert_base_baseline.json"), num_hidden_layers=2), num_labels=13, batch=2,
                             n_tok=38, n_reg=101, stride={"vision_prediction": 16, "linguisic_prediction": 97}),
}


def _json(name):
    import json
    with open(os.path.join(synth.CONFIG_DIR, name), "r", encoding="utf-8") as f:
        return json.load(f)


def config(case):
    """A plain attribute bag of the case's config (what both the reference's and the native classes read)."""
    return types.SimpleNamespace(**CASES[case]["cfg"]())


def path(case):
    return os.path.join(GOLDEN_DIR, case + ".npz")


def make_state_dict(shapes, seed=4321):
    """{name: tensor} for the (name, shape) list of a state_dict: matrices and biases ~ N(0, 0.02), LayerNorm weights
    ~ 1 + N(0, 0.1), LayerNorm biases ~ N(0, 0.1), weight_g ~ 1 + |N(0, 0.1)| (oracle/synth.py's distributions, per-tensor
    generators seeded by crc32(name) ^ seed). The tied decoder weight IS the word table."""
    sd = {}
    for name, shape in shapes:
        if name == "cls.predictions.decoder.weight":
            sd[name] = sd["bert.embeddings.word_embeddings.weight"]
            continue
        g = torch.Generator().manual_seed((zlib.crc32(name.encode()) ^ seed) & 0x7FFFFFFF)
        x = torch.randn(tuple(shape), generator=g, dtype=torch.float32)
        if "LayerNorm.weight" in name:
            x.mul_(0.1).add_(1.0)
        elif "LayerNorm.bias" in name:
            x.mul_(0.1)
        elif name.endswith("weight_g"):
            x = x.mul_(0.1).abs_().add_(1.0)
        else:
            x.mul_(0.02)
        sd[name] = x
    return sd


def make_inputs(case, seed=11):
    """Ragged text and image masks, two token types, at least one input id 0 inside the text mask."""
    c = CASES[case]
    cfg = c["cfg"]()
    B, T, R = c["batch"], c["n_tok"], c["n_reg"]
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, cfg["vocab_size"], (B, T), generator=g)
    ids[0, 2] = 0
    ids[B - 1, 1] = 0
    tl = torch.randint(max(3, T // 2), T + 1, (B,), generator=g)
    rl = torch.randint(max(2, R // 2), R + 1, (B,), generator=g)
    tl[0], rl[B - 1] = T, R
    mask = (torch.arange(T)[None, :] < tl[:, None]).long()
    imask = (torch.arange(R)[None, :] < rl[:, None]).long()
    seg = (torch.arange(T)[None, :] >= (tl[:, None] + 1) // 2).long() * mask
    feat = torch.rand(B, R, 2048, generator=g) * 2.0 * imask[:, :, None].float()
    loc = torch.rand(B, R, 5, generator=g)
    return dict(input_ids=ids, image_feat=feat, image_loc=loc, token_type_ids=seg, attention_mask=mask,
                image_attention_mask=imask)


def forward_args(x):
    return (x["input_ids"], x["image_feat"], x["image_loc"], x["token_type_ids"], x["attention_mask"],
            x["image_attention_mask"])


def weighted_loss(outs, image_mask):
    """sum_i w_i * out_i over the seven outputs (in HEADS order), vision_logit through the image mask."""
    total = 0.0
    for name, o in zip(HEADS, outs):
        w = LOSS_WEIGHTS[name]
        total = total + ((o * image_mask.to(o.dtype).unsqueeze(2)).sum() if w is None else (w * o).sum())
    return total


def sample(case, name, t):
    step = CASES[case].get("stride", {}).get(name, 1)
    return t[..., ::step] if step > 1 else t
