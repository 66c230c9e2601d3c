"""Import-name shim for the reference's reduced-precision branch (train_concap.py:443-461, train_tasks.py the same block):

    from apex.optimizers import FP16_Optimizer, FusedAdam
    optimizer = FusedAdam(grouped_parameters, lr=..., bias_correction=False, max_grad_norm=1.0)
    optimizer = FP16_Optimizer(optimizer, dynamic_loss_scale=True)      # or static_loss_scale=...
    ...
    model.half()                    # train_concap.py:504-505
    optimizer.backward(loss)        # :570-571
    optimizer.step(); optimizer.zero_grad()

NVIDIA apex does not exist on ROCm images. On this package that mode is the bf16 stream: bfloat16
activations / gradients, fp32 master weights that the native AdamW updates directly - bf16 has fp32's exponent range, so
there is no loss scale to manage: `backward(loss)` is `loss.backward()` and `loss_scale` reads 1.0.
`max_grad_norm` (FusedAdam's global-norm clipping, which apex applies through FP16_Optimizer's combined scale) is native
(vilbert.optim.AdamW, csrc/optimizer.hip): one norm pass over every gradient the step updates - arena slice or not, whoever
owns the arena, whatever the order in which optimizer and DistributedDataParallel were built - leaves the clip coefficient
on the device and the update kernel multiplies it in as it loads the gradients; `.grad` is not rewritten (apex passes its
scale to the kernel the same way). As in apex, a step whose gradients hold an inf / NaN is skipped - parameters and moments
keep their bits - and `FP16_Optimizer.overflow` reports it.

`FusedLAMB` stands next to `FusedAdam` as it does in apex: the optimizer for pre-training at a global batch of thousands of
samples, on the native LAMB step (vilbert.optim.LAMB, csrc/lamb.hip), inside the same `FP16_Optimizer`.
"""
import torch

from vilbert.optim import LAMB, AdamW


class FusedAdam(AdamW):
    """apex.optimizers.FusedAdam's constructor on the native multi-tensor AdamW (csrc/optimizer.hip). apex's update
    p -= step_size * (m / (sqrt(v) + eps) + weight_decay * p) is AdamW's decoupled form with the decay scaled by the same
    step size; eps_inside_sqrt is not offered by the native kernel."""

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-8, eps_inside_sqrt=False,
                 weight_decay=0.0, max_grad_norm=0.0, amsgrad=False):
        if amsgrad:
            raise RuntimeError("FusedAdam does not support the AMSGrad variant.")
        if eps_inside_sqrt:
            raise RuntimeError("FusedAdam (MI355X-native): eps_inside_sqrt is not supported")
        super(FusedAdam, self).__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                        correct_bias=bool(bias_correction), max_grad_norm=max_grad_norm,
                                        skip_nonfinite=True)

    def clip_(self):
        """In-place global-norm clipping of the `.grad` tensors of this optimizer's parameters (torch, eager); returns
        the norm (a device scalar) or None. step() does NOT call it - it clips inside the native update without touching
        the gradients; this stays for callers that want clipped `.grad` tensors. It goes through the parameters, not a
        gradient arena, so it does not matter who owns the arena."""
        if self.max_grad_norm <= 0.0:
            return None
        params = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        return torch.nn.utils.clip_grad_norm_(params, self.max_grad_norm) if params else None

    def step(self, closure=None, **_apex_kwargs):      # (apex passes grads / output_params / scale / grad_norms)
        return super(FusedAdam, self).step(closure)


class FusedLAMB(LAMB):
    """apex.optimizers.FusedLAMB's constructor on the native LAMB step (vilbert.optim.LAMB, csrc/lamb.hip): the optimizer
    to select when pre-training at a global batch of thousands of samples. As FusedAdam above, a step whose gradients hold
    an inf / NaN is skipped. Differences from apex, whose bits nothing here is pinned against (apex does not exist on ROCm
    images): the step count - and with it the bias correction - is kept per tensor, not per group (a tensor that misses a
    gradient falls behind, as in every optimizer of this package); the clip coefficient is the package's own,
    min(1, max_grad_norm / (||g|| + 1e-6)) of ``torch.nn.utils.clip_grad_norm_``, where apex divides by
    ||g|| / max_grad_norm when that exceeds 1; fp16 parameter lists and AMSGrad are not offered. ``set_grad_none`` is the default of
    ``zero_grad()``'s ``set_to_none``."""

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01,
                 amsgrad=False, adam_w_mode=True, grad_averaging=True, set_grad_none=True, max_grad_norm=1.0,
                 use_nvlamb=False):
        if amsgrad:
            raise RuntimeError("FusedLAMB does not support the AMSGrad variant.")
        super(FusedLAMB, self).__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                        bias_correction=bias_correction, grad_averaging=grad_averaging,
                                        adam_w_mode=adam_w_mode, use_nvlamb=use_nvlamb, max_grad_norm=max_grad_norm,
                                        skip_nonfinite=True)
        self.set_grad_none = bool(set_grad_none)

    _PICKLED = LAMB._PICKLED + ("set_grad_none",)

    def zero_grad(self, set_to_none=None):
        super(FusedLAMB, self).zero_grad(set_to_none=self.set_grad_none if set_to_none is None else set_to_none)

    def step(self, closure=None, **_apex_kwargs):      # (apex passes grads / output_params / scale / grad_norms)
        return super(FusedLAMB, self).step(closure)


class FP16_Optimizer(torch.optim.Optimizer):
    """apex.optimizers.FP16_Optimizer's public face around a FusedAdam (or any optimizer of this package). The wrapped
    optimizer already holds the fp32 master weights (the model's own parameters: `model.half()` leaves them fp32 here), so
    there are no fp16 copies to keep in sync and no scaled gradients to unscale. A torch Optimizer by type (the scripts hand
    it to `WarmupLinearSchedule`, whose base class insists on one): it SHARES the wrapped optimizer's parameter-group
    dictionaries and state."""

    def __init__(self, init_optimizer, static_loss_scale=1.0, dynamic_loss_scale=False, dynamic_loss_args=None, verbose=True):
        super(FP16_Optimizer, self).__init__(init_optimizer.param_groups, init_optimizer.defaults)
        assert all(a is b for a, b in zip(self.param_groups, init_optimizer.param_groups))     # the same dict objects
        self.optimizer = init_optimizer
        self.state = init_optimizer.state
        self.dynamic_loss_scale = bool(dynamic_loss_scale)
        self.static_loss_scale = static_loss_scale
        self.cur_scale = 1.0

    @property
    def overflow(self):
        """Whether the last step was skipped because of non-finite gradients. Read lazily from the device flag the norm
        kernel wrote: step() itself never synchronises, reading this does."""
        skipped = getattr(self.optimizer, "last_step_skipped", None)
        return bool(skipped()) if skipped is not None else False

    @property
    def loss_scale(self):
        return self.cur_scale

    def zero_grad(self, set_grads_to_None=True):
        self.optimizer.zero_grad()

    def backward(self, loss):
        loss.backward()

    def step(self, closure=None):
        return self.optimizer.step(closure)

    def state_dict(self):
        return {"dynamic_loss_scale": self.dynamic_loss_scale, "cur_scale": self.cur_scale,
                "optimizer_state_dict": self.optimizer.state_dict()}

    def load_state_dict(self, state_dict):
        self.optimizer.load_state_dict(state_dict["optimizer_state_dict"])
