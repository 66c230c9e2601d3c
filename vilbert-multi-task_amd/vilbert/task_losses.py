"""Loss modules and answer score of the fine-tuning heads on the native kernels (csrc/task_loss.hip, csrc/loss.hip).

The reference's trainer takes its criteria from `vilbert.task_utils.LossMap` - `nn.BCEWithLogitsLoss(reduction="mean")` for
eight of the twelve tasks, `nn.CrossEntropyLoss()` for the retrieval / VCR ones - and scores three head types with
`compute_score_with_logits` (task_utils.py:25-28, 325-374, 618-623). The classes here ARE those torch modules (subclasses:
`isinstance`, `state_dict`, pickling by reference all keep working) and take the native path exactly where the kernels
compute the same thing: fp32 HIP tensors, mean reduction, no weights. Everything else - CPU tensors, other dtypes, other
reductions, weights - is `super().forward`, bit for bit what torch computes. vilbert/__init__.py rebinds the three names
in the reference's module after its body has run."""
import torch
import torch.nn as nn

from . import ops
from .autograd_ops import BCEWithLogitsFn, CrossEntropyFn


# The output of VILBertForVLTasks.forward that ForwardModelsTrain reads per `task_cfg[task]["type"]` (task_utils.py:325-374):
# what a trainer passes to `model.set_active_heads([...])` so that a step computes that head alone. Also bound into the
# reference's module as `vilbert.task_utils.HEAD_OF_TASK_TYPE`.
HEAD_OF_TASK_TYPE = {
    "VL-classifier": "vil_prediction",
    "VL-classifier-GQA": "vil_prediction_gqa",
    "VL-logit": "vil_logit",
    "V-logit": "vision_logit",
    "V-logit-mc": "vision_logit",
    "VL-binary-classifier": "vil_binary_prediction",
    "VL-tri-classifier": "vil_tri_prediction",
}


def _fp32_hip(t):
    return torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32


class BCEWithLogitsLoss(nn.BCEWithLogitsLoss):
    """nn.BCEWithLogitsLoss whose mean reduction of fp32 HIP tensors is one deterministic reduction forward (two launches
    at most) and one launch backward, instead of torch's elementwise + mean pair in each direction."""

    def _native(self, input, target):
        return (_fp32_hip(input) and _fp32_hip(target) and target.shape == input.shape and target.device == input.device
                and self.reduction == "mean" and self.weight is None and self.pos_weight is None
                and not target.requires_grad and input.numel() > 0)

    def forward(self, input, target):
        if self._native(input, target):
            return BCEWithLogitsFn.apply(input, target)
        return super().forward(input, target)


class CrossEntropyLoss(nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss whose plain case - fp32 HIP logits [rows, n], int64 class labels [rows], mean reduction, no class
    weights, no label smoothing - runs on the cross-entropy kernels of the pre-training heads (CrossEntropyFn). A label
    outside [0, n) other than ignore_index gives a NaN loss there (torch raises a device-side assert)."""

    def _native(self, input, target):
        return (_fp32_hip(input) and input.dim() == 2 and input.numel() > 0 and torch.is_tensor(target)
                and target.dtype == torch.int64 and target.dim() == 1 and target.shape[0] == input.shape[0]
                and target.device == input.device and self.reduction == "mean" and self.weight is None
                and self.label_smoothing == 0.0)

    def forward(self, input, target):
        if self._native(input, target):
            return CrossEntropyFn.apply(input, target, self.ignore_index)
        return super().forward(input, target)


def _native_score(logits, labels):
    return (_fp32_hip(logits) and _fp32_hip(labels) and labels.shape == logits.shape and labels.device == logits.device
            and logits.numel() > 0 and not labels.requires_grad and (logits.dim() == 2 or (logits.dim() == 3 and logits.shape[2] == 1)))


def row_argmax_pick(logits, labels):
    """(idx int64 [rows], picked fp32 [rows]): per row of [rows, n] (or [rows, n, 1]) the lowest index of the maximum of the
    logits and the label at that index - `torch.max(logits, 1)[1]` and `labels.gather(1, idx)` in one launch on HIP tensors,
    those two torch calls elsewhere."""
    if _native_score(logits, labels):
        idx, picked, _ = ops.argmax_pick(logits.detach(), labels.detach())
        return idx, picked
    if logits.dim() == 3 and logits.shape[2] == 1:
        logits, labels = logits.squeeze(2), labels.squeeze(2)
    idx = torch.max(logits, 1)[1].data
    return idx, labels.gather(1, idx.view(-1, 1)).view(-1)


def compute_score_with_logits(logits, labels):
    """task_utils.py:618-623: the one-hot of the row arg-max times the (soft) labels, in the labels' shape. One launch on
    fp32 HIP tensors; otherwise upstream's torch arithmetic, with the one-hot made on the labels' device."""
    if _native_score(logits, labels):
        return ops.argmax_pick(logits.detach(), labels.detach(), want_dense=True)[2]
    logits = torch.max(logits, 1)[1].data  # argmax
    one_hots = torch.zeros(*labels.size(), device=labels.device)
    one_hots.scatter_(1, logits.view(-1, 1), 1)
    scores = one_hots * labels
    return scores
