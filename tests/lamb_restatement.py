"""A restatement of the LAMB step (You et al. 2020; vilbert.optim.LAMB, csrc/lamb.hip) as a per-tensor loop of plain torch
operations in any dtype on any device, with the clipping / gradient scale / overflow skip of the optimizers' base class. Test
infrastructure: run in float64 it is the yardstick of tests/test_lamb_gpu.py, run in float32 on the CPU it gives the distance
those tests' bounds are built on (tests/test_lamb.py measures and records it), and tools/lamb_step_bench.py times it on the
device as the per-tensor torch loop a trainer would otherwise run.

One step, over the tensors that have a gradient (a tensor without one is left out and its own step count t stays):
    coef = grad_scale * min(1, max_grad_norm / (|grad_scale| * ||all g|| + 1e-6))       (1 when nothing is clipped or scaled)
    skip_nonfinite and ||all g||^2 not finite in fp32: nothing changes but the step counts and the skip counter
    g = coef * gradient;   L2 mode: g += wd * p
    m <- beta1 m + beta3 g                      beta3 = 1 - beta1 with grad_averaging, else 1
    v <- beta2 v + (1 - beta2) g g
    u = (m / bc1) / (sqrt(v / bc2) + eps)       bc = 1 - beta^t with bias_correction, else 1
    adam_w_mode: u += wd * p
    r = ||p|| / ||u||  if (use_nvlamb or wd != 0) and ||p|| > 0 and ||u|| > 0, else 1
    p <- p - lr r u
The scalars are Python floats (double), the tensor arithmetic and the norms run in the tensors' dtype.
"""
import math

import torch


class Restatement(object):
    """`tensors`: initial values (cloned; with clone=False they are updated in place); `groups`: dicts with "idx" (indices
    into `tensors`), "lr", "weight_decay"."""

    def __init__(self, tensors, groups, betas=(0.9, 0.999), eps=1e-6, bias_correction=True, grad_averaging=True,
                 adam_w_mode=True, use_nvlamb=False, max_grad_norm=1.0, grad_scale=1.0, skip_nonfinite=False, clone=True):
        self.p = [t.detach().clone() if clone else t.detach() for t in tensors]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.t = [0] * len(self.p)
        self.groups = [dict(g) for g in groups]
        self.betas, self.eps, self.bias_correction, self.grad_averaging = betas, eps, bias_correction, grad_averaging
        self.adam_w_mode, self.use_nvlamb = adam_w_mode, use_nvlamb
        self.max_grad_norm, self.grad_scale, self.skip_nonfinite = max_grad_norm, grad_scale, skip_nonfinite
        self.skipped = 0
        self.order, self.trust = [], {}        # tensors of the last applied step in walking order; tensor -> r (float)
        self.grad_norm, self.coef = None, 1.0

    def _coefficient(self, used):
        """(coef, finite) of the base class's norm pass over the gradients of this step."""
        if not (self.max_grad_norm > 0.0 or self.grad_scale != 1.0 or self.skip_nonfinite):
            return 1.0, True
        ss = float(torch.stack([g.pow(2).sum() for g in used]).sum())
        finite = math.isfinite(float(torch.tensor(ss, dtype=torch.float32)))
        self.grad_norm = abs(self.grad_scale) * math.sqrt(ss) if ss >= 0.0 else float("nan")
        clip = 1.0
        if self.max_grad_norm > 0.0:
            clip = min(1.0, self.max_grad_norm / (self.grad_norm + 1e-6)) if self.grad_norm == self.grad_norm else float("nan")
        # the device keeps the coefficient as one number of the working precision
        return float(torch.tensor(self.grad_scale * clip, dtype=used[0].dtype)), finite

    @torch.no_grad()
    def step(self, grads):
        """`grads`: one tensor (or None) per tensor, in the tensors' dtype."""
        beta1, beta2 = self.betas
        walk = [(i, group) for group in self.groups for i in group["idx"] if grads[i] is not None]
        if not walk:
            return
        for i, _group in walk:
            self.t[i] += 1
        self.coef, finite = self._coefficient([grads[i] for i, _g in walk])
        if self.skip_nonfinite and not finite:
            self.skipped += 1
            return
        self.order = [i for i, _g in walk]
        for i, group in walk:
            p, m, v, t = self.p[i], self.m[i], self.v[i], self.t[i]
            lr, wd = group["lr"], group["weight_decay"]
            g = grads[i] * self.coef
            if not self.adam_w_mode:
                g = g + wd * p
            m.mul_(beta1).add_(g, alpha=(1.0 - beta1) if self.grad_averaging else 1.0)
            v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
            bc1 = 1.0 - beta1 ** t if self.bias_correction else 1.0
            bc2 = 1.0 - beta2 ** t if self.bias_correction else 1.0
            u = (m / bc1) / ((v / bc2).sqrt() + self.eps)
            if self.adam_w_mode:
                u = u + wd * p
            r = 1.0
            if self.use_nvlamb or wd != 0:
                # (sum of squares through torch.sum, which adds pairwise: Tensor.norm() of an fp32 CPU tensor accumulates
                # in sequence and is off by 6e-5 on 196,608 values of about equal size)
                pn, un = float(p.pow(2).sum().sqrt()), float(u.pow(2).sum().sqrt())
                if pn > 0.0 and un > 0.0:
                    r = pn / un
            self.trust[i] = r
            p.add_(u, alpha=-lr * r)

    def state_dict(self, **group_extras):
        """The layout torch.optim.Optimizer.state_dict() gives vilbert.optim.LAMB."""
        index, packed = 0, []
        for g in self.groups:
            packed.append(dict({"lr": g["lr"], "betas": self.betas, "eps": self.eps, "weight_decay": g["weight_decay"],
                                "bias_correction": self.bias_correction, "grad_averaging": self.grad_averaging,
                                "params": list(range(index, index + len(g["idx"])))}, **group_extras))
            index += len(g["idx"])
        order = [i for g in self.groups for i in g["idx"]]
        state = {k: {"step": self.t[i], "exp_avg": self.m[i].clone(), "exp_avg_sq": self.v[i].clone()}
                 for k, i in enumerate(order) if self.t[i] > 0}
        return {"state": state, "param_groups": packed}


# ---- the case of the trajectory tests (tests/test_lamb.py measures its fp32 distance, tests/test_lamb_gpu.py runs it) -----
CHUNK = 65536
# 0: one element; 1: five elements, on the device an odd-offset view (scalar path); 2: two chunks, the second with one 16-byte
# access and a 3-element scalar tail; 3: three full chunks (its neighbours check first_chunk); 4: an all-zero parameter with
# a non-zero gradient (||p|| = 0 on its first step); 5: zero gradients on every step, so zero moments, in the group without
# decay (||u|| = 0, p never moves); 6: a tensor of the group without decay (r = 1 exactly unless use_nvlamb);
# 7: misses its gradient on two steps. 268,598 elements in all.
SIZES = (1, 5, CHUNK + 7, 3 * CHUNK, 1021, 300, 4099, 1021)
ODD, ZERO_PARAM, ZERO_GRAD, NO_DECAY, LAGGING = 1, 4, 5, 6, 7
GROUPS = ({"idx": [0, 1, 2, 3, 4, 7], "lr": 1e-2, "weight_decay": 0.01}, {"idx": [5, 6], "lr": 1e-3, "weight_decay": 0.0})
MISSING = {(4, LAGGING), (9, LAGGING)}         # (1-based step, tensor): no gradient
STEPS = 12
MAX_GRAD_NORM = 1.0
# gradient scale per step: ||randn|| over the 268,298 elements with a non-zero gradient is about 518, so the global norm is
# about 52 on the odd steps (clipped by 52) and about 0.5 on the even ones (not clipped)
GRAD_SCALES = (0.1, 1e-3)
CONFIGS = [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False)]   # adam_w_mode, bias_correction, grad_averaging


def lr_factor(step):
    """The shrinking learning rate of the case (1-based step)."""
    return 1.0 - 0.05 * (step - 1)


def inputs(seed=20200, steps=STEPS, missing=MISSING, scales=GRAD_SCALES):
    """p0 (list of fp32 tensors) and grads[step][tensor] (fp32 tensor or None), deterministic."""
    g = torch.Generator().manual_seed(seed)
    p0 = [torch.randn(n, generator=g) for n in SIZES]
    p0[ZERO_PARAM].zero_()
    grads = []
    for step in range(1, steps + 1):
        row = [torch.randn(n, generator=g) * scales[(step - 1) % len(scales)] for n in SIZES]
        row[ZERO_GRAD].zero_()
        grads.append([None if (step, i) in missing else t for i, t in enumerate(row)])
    return p0, grads


def run_case(p0, grads, groups, dtype, factor=None, device="cpu", **options):
    """The whole trajectory in `dtype`; returns the Restatement."""
    r = Restatement([t.to(device=device, dtype=dtype) for t in p0], groups, **options)
    base = [g["lr"] for g in r.groups]
    for k, row in enumerate(grads):
        if factor is not None:
            for g, lr in zip(r.groups, base):
                g["lr"] = lr * factor(k + 1)
        r.step([None if t is None else t.to(device=device, dtype=dtype) for t in row])
    return r
