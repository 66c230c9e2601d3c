"""A restatement of the two rectified-Adam variants the fine-tuning script offers (`--optim RAdam`: the classes `RAdam` and
`PlainRAdam` of the reference's vilbert/optimization.py), as a per-tensor loop of plain torch operations in any dtype on any
device. Test infrastructure: tests/test_radam.py pins it (run in fp32) against a trajectory recorded from the real classes
(tests/golden/radam_trajectory.npz, written by tests/golden/make_radam_golden.py); run in float64 it is the yardstick of the
GPU tests (tests/test_radam_gpu.py), and tools/radam_step_bench.py times it on the device as the stand-in for the reference's
step (the reference itself is not present where the GPU is).

Per tensor at its own 1-based step count t (a tensor without a gradient is skipped and its count stays):
    v <- beta2 v + (1 - beta2) g g
    m <- beta1 m + (1 - beta1) g
    N_max = 2 / (1 - beta2) - 1,   N = N_max - 2 t beta2^t / (1 - beta2^t)
    p <- p - wd lr p                                                     (if wd != 0)
    N >= 5:  p <- p - s m / (sqrt(v) + eps),  s = lr sqrt((1 - beta2^t) (N-4)/(N_max-4) (N-2)/N N_max/(N_max-2)) / (1 - beta1^t)
    else:    p <- p - s m,                    s = lr / (1 - beta1^t)
`RAdam` keeps ten slots [t, N, s] indexed by t mod 10 and reuses a slot whose t matches - so s carries the learning rate of
whichever group computed it first; `PlainRAdam` computes s from each group's own lr every time. The scalars are Python floats
(double), the tensor arithmetic runs in the tensors' dtype.
"""
import math

import torch


class Restatement(object):
    """`tensors`: initial values (cloned; with clone=False they are updated in place); `groups`: dicts with "idx" (indices
    into `tensors`), "lr", "weight_decay"."""

    def __init__(self, tensors, groups, plain=False, betas=(0.9, 0.999), eps=1e-8, clone=True):
        self.p = [t.detach().clone() if clone else t.detach() for t in tensors]
        self.m = [torch.zeros_like(t) for t in self.p]
        self.v = [torch.zeros_like(t) for t in self.p]
        self.t = [0] * len(self.p)
        self.groups = [dict(g) for g in groups]
        self.plain, self.betas, self.eps = plain, betas, eps
        self.slots = [[None, None, None] for _ in range(10)]
        self.applied = []                      # (tensor index, t, N, s) of every update, in order

    def _scalars(self, t, lr):
        beta1, beta2 = self.betas
        if not self.plain and self.slots[t % 10][0] == t:
            return self.slots[t % 10][1], self.slots[t % 10][2]
        b2t = beta2 ** t
        n_max = 2.0 / (1.0 - beta2) - 1.0
        n = n_max - 2.0 * t * b2t / (1.0 - b2t)
        s = lr / (1.0 - beta1 ** t)
        if n >= 5:
            s = lr * math.sqrt((1.0 - b2t) * (n - 4.0) / (n_max - 4.0) * (n - 2.0) / n * n_max / (n_max - 2.0)) / (1.0 - beta1 ** t)
        if not self.plain:
            self.slots[t % 10] = [t, n, s]
        return n, s

    @torch.no_grad()
    def step(self, grads):
        """`grads`: one tensor (or None) per tensor, in the tensors' dtype."""
        beta1, beta2 = self.betas
        for group in self.groups:
            for i in group["idx"]:
                g = grads[i]
                if g is None:
                    continue
                p, m, v = self.p[i], self.m[i], self.v[i]
                v.mul_(beta2).addcmul_(g, g, value=1.0 - beta2)
                m.mul_(beta1).add_(g, alpha=1.0 - beta1)
                self.t[i] += 1
                n, s = self._scalars(self.t[i], group["lr"])
                self.applied.append((i, self.t[i], n, s))
                if group["weight_decay"] != 0:
                    p.add_(p, alpha=-group["weight_decay"] * group["lr"])
                if n >= 5:
                    p.addcdiv_(m, v.sqrt().add_(self.eps), value=-s)
                else:
                    p.add_(m, alpha=-s)

    def state_dict(self):
        """The layout torch.optim.Optimizer.state_dict() gives the reference's classes."""
        index, packed = 0, []
        for g in self.groups:
            packed.append({"lr": g["lr"], "betas": self.betas, "eps": self.eps, "weight_decay": g["weight_decay"],
                           "params": list(range(index, index + len(g["idx"])))})
            index += len(g["idx"])
        order = [i for g in self.groups for i in g["idx"]]
        state = {k: {"step": self.t[i], "exp_avg": self.m[i].clone(), "exp_avg_sq": self.v[i].clone()}
                 for k, i in enumerate(order) if self.t[i] > 0}
        return {"state": state, "param_groups": packed}


# ---- the case of the golden fixture (tests/golden/radam_trajectory.npz) ----------------------------------------------
GOLDEN_STEPS = 12
GOLDEN_SIZES = (7, 33, 5)
GOLDEN_GROUPS = ({"idx": [0, 1], "lr": 1e-3, "weight_decay": 0.01}, {"idx": [2], "lr": 1e-5, "weight_decay": 0.0})
GOLDEN_MISSING = {(4, 1), (9, 1)}          # (1-based step, tensor): no gradient - the tensor's own count falls behind


def golden_lr_factor(step):
    """Learning-rate schedule of the fixture (1-based step): a lagging tensor then meets a slot filled under an older lr."""
    return 1.0 - 0.05 * (step - 1)


def golden_inputs():
    """p0 (list of fp32 tensors) and grads[step][tensor] (fp32 tensor or None), deterministic."""
    g = torch.Generator().manual_seed(20191)
    p0 = [torch.randn(n, generator=g) for n in GOLDEN_SIZES]
    grads = []
    for step in range(1, GOLDEN_STEPS + 1):
        row = [torch.randn(n, generator=g) * 0.1 for n in GOLDEN_SIZES]
        grads.append([None if (step, i) in GOLDEN_MISSING else t for i, t in enumerate(row)])
    return p0, grads


def run_case(p0, grads, groups, plain, dtype, lr_factor=None, device="cpu", betas=(0.9, 0.999)):
    """The whole trajectory in `dtype`; returns the Restatement."""
    r = Restatement([t.to(device=device, dtype=dtype) for t in p0], groups, plain=plain, betas=betas)
    base = [g["lr"] for g in r.groups]
    for k, row in enumerate(grads):
        if lr_factor is not None:
            for g, lr in zip(r.groups, base):
                g["lr"] = lr * lr_factor(k + 1)
        r.step([None if t is None else t.to(device=device, dtype=dtype) for t in row])
    return r
