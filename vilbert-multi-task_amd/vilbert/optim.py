"""AdamW + warm-up schedules with the semantics of pytorch-transformers 1.0.0 (the optimizer the reference
imports: train_concap.py:27,465-476; train_tasks.py:26-30,426-437), the update itself being ONE native
multi-tensor launch (csrc/optimizer.hip) instead of ~6 torch kernels per parameter tensor.

Also importable as ``pytorch_transformers.optimization`` (shim package next to this one) so that the
unchanged reference scripts pick it up.

RAdam / PlainRAdam (the reference's own ``vilbert/optimization.py``, ``train_tasks.py --optim RAdam``) run on the same
plumbing with a kernel of their own (``vbo_radam_step``); ``import vilbert.optimization`` hands them out under the
reference's import path (vilbert/__init__.py: _OptimizationFinder).

LAMB (layer-wise trust ratios, for pre-training at a large global batch) runs on the same plumbing as two launches with
per-tensor norms (csrc/lamb.hip, ``vbl_lamb_step``); ``apex.optimizers.FusedLAMB`` is apex's constructor on top of it.
"""
import ctypes
import math

import numpy as np
import torch
from torch.optim import Optimizer
from torch.optim.lr_scheduler import LambdaLR

from . import _native as N

CHUNK_ELEMS = 64 * 1024

_TABLE_DTYPE = np.dtype([
    ("param", "<u8"), ("grad", "<u8"), ("exp_avg", "<u8"), ("exp_avg_sq", "<u8"), ("numel", "<i8"),
    ("step_size", "<f4"), ("beta1", "<f4"), ("beta2", "<f4"), ("eps", "<f4"), ("decay", "<f4"),
    ("reserved", "<f4")])
_RADAM_DTYPE = np.dtype([
    ("step_size", "<f4"), ("decay", "<f4"), ("beta1", "<f4"), ("beta2", "<f4"), ("one_minus_beta1", "<f4"),
    ("one_minus_beta2", "<f4"), ("eps", "<f4"), ("rectified", "<i4")])
_LAMB_DTYPE = np.dtype([
    ("lr", "<f4"), ("weight_decay", "<f4"), ("beta1", "<f4"), ("beta2", "<f4"), ("beta3", "<f4"), ("one_minus_beta2", "<f4"),
    ("bc1", "<f4"), ("bc2", "<f4"), ("eps", "<f4"), ("adam_w_mode", "<i4"), ("apply_trust", "<i4"), ("first_chunk", "<i4"),
    ("n_chunks", "<i4")])


def _check_clip_args(max_grad_norm, grad_scale):
    if not (0.0 <= float(max_grad_norm) < math.inf):
        raise ValueError("Invalid max_grad_norm: {} - should be finite and >= 0.0 (0 = no clipping)".format(max_grad_norm))
    if not math.isfinite(float(grad_scale)):
        raise ValueError("Invalid grad_scale: {} - should be finite".format(grad_scale))


def _check_adam_args(lr, betas, eps):
    if lr < 0.0:
        raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
    if not 0.0 <= betas[0] < 1.0:
        raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[0]))
    if not 0.0 <= betas[1] < 1.0:
        raise ValueError("Invalid beta parameter: {} - should be in [0.0, 1.0[".format(betas[1]))
    if not 0.0 <= eps:
        raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(eps))


class _MultiTensorOptimizer(Optimizer):
    """What the native optimizers share: the gradient arena, the launch tables (one vb_adamw_tensor row per tensor, chunk
    lists on the device, uploaded through pinned memory without a host synchronisation), the fused global-norm clipping /
    gradient scale / overflow skip (vbx_grad_norm leaves a device-resident state the update kernel reads), graph capture
    and replay, and the weights epoch. A subclass supplies its hyper-parameters (`_fill_hyper`) and its launch (`_launch`)
    and may append a second per-tensor table to the upload (`_EXTRA_DTYPE`: its rows follow the vb_adamw_tensor rows in
    the same device buffer, `_extra_ptr(plan)` is their address).

    ``max_grad_norm`` > 0 clips the global norm of all gradients of the step (the coefficient of
    ``torch.nn.utils.clip_grad_norm_``), ``grad_scale`` multiplies every gradient (e.g. 1 / world size behind a SUM
    exchange; the norm is that of the scaled gradients), ``skip_nonfinite`` leaves parameters and moments untouched when a
    gradient is inf / NaN (or the fp32 sum of squares overflows). All three are native (csrc/optimizer.hip): one norm pass
    over the gradients, a device-resident coefficient the update kernel multiplies in as it loads them - no host
    synchronisation, capturable by GraphedTrainStep. Unlike ``clip_grad_norm_`` the ``.grad`` tensors are NOT modified
    (apex's FusedAdam passes its scale the same way). The norm covers exactly the tensors the step updates, whether their
    gradient is a slice of the gradient arena or a tensor of its own. ``state["step"]`` advances on the host also for a
    skipped step (the skip is decided on the device). With the defaults step() is the plain launch: no norm pass, no extra
    buffers. The three values are plain attributes; a captured step keeps the values it was captured with."""

    _NAME = "optimizer"
    _EXTRA_DTYPE = None

    def _init_native(self, max_grad_norm, grad_scale, skip_nonfinite):
        """Before Optimizer.__init__: the three clipping attributes."""
        _check_clip_args(max_grad_norm, grad_scale)
        self.max_grad_norm, self.grad_scale, self.skip_nonfinite = float(max_grad_norm), float(grad_scale), bool(skip_nonfinite)
        self._grad_state = None          # device floats written by vbx_grad_norm (_native.GRAD_STATE_*), one per optimizer

    def _init_plan(self):
        """After Optimizer.__init__ (the parameter groups exist)."""
        self._plan_key, self._plan = None, None
        self._arena = None
        self._ensure_arena()

    def __setstate__(self, state):
        """Unpickling (torch.optim.Optimizer pickles defaults, state and groups only): the clipping attributes come back
        at their defaults, the launch plan is rebuilt at the next step."""
        super(_MultiTensorOptimizer, self).__setstate__(state)
        if not hasattr(self, "_grad_state"):
            self._init_native(0.0, 1.0, False)
            self._init_plan()

    def _fill_hyper(self, plan, entries):
        """Per-step hyper-parameter columns of the table(s), from the groups and each tensor's own step count."""
        raise NotImplementedError

    def _launch(self, plan, state, skip):
        """Enqueue the update on the current stream; `state` is the device state of the norm pass, None = the plain step."""
        raise NotImplementedError

    def _ensure_arena(self):
        """Gives the optimizer's parameters a gradient arena (arena.py: gradients at fixed addresses in one flat
        buffer, zero-filled once per backward, written in place by the backward kernels) unless something else - the
        data-parallel wrapper - already manages them. Done at construction when the parameters are on the device,
        else at the first step()."""
        if self._arena is not None:
            return
        from . import arena
        params = [p for g in self.param_groups for p in g["params"] if p.requires_grad]
        if not params or not all(p.is_cuda and p.dtype == torch.float32 for p in params):
            return
        if all(arena.lookup(p) is not None for p in params):
            return
        self._arena = arena.GradArena(list(reversed(params)))

    def _build_plan(self, entries, device):
        """Static part of the launch tables for this set of tensors: chunk lists on the device and a
        host-side structured array whose grad / hyper-parameter columns are refreshed every step."""
        tab = np.zeros(len(entries), dtype=_TABLE_DTYPE)
        assert tab.dtype.itemsize == ctypes.sizeof(N.AdamWTensor)
        chunk_t, chunk_o = [], []
        for i, (p, st, _g) in enumerate(entries):
            tab["param"][i], tab["exp_avg"][i], tab["exp_avg_sq"][i] = p.data_ptr(), st["exp_avg"].data_ptr(), \
                st["exp_avg_sq"].data_ptr()
            tab["numel"][i] = p.numel()
            for off in range(0, p.numel(), CHUNK_ELEMS):
                chunk_t.append(i)
                chunk_o.append(off)
        extra = None if self._EXTRA_DTYPE is None else np.zeros(len(entries), dtype=self._EXTRA_DTYPE)
        # two pinned staging copies of the table(s) (the host may run one step ahead of the device) + events
        nbytes = tab.nbytes + (0 if extra is None else extra.nbytes)
        pinned = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        return dict(tab=tab, extra=extra, n_chunks=len(chunk_t), pinned=pinned, events=[None, None], turn=0,
                    dev_tab=torch.empty(nbytes, dtype=torch.uint8, device=device),
                    chunk_tensor=torch.tensor(chunk_t, dtype=torch.int32, device=device),
                    chunk_off=torch.tensor(chunk_o, dtype=torch.int64, device=device))

    @staticmethod
    def _stage(plan, k):
        """Host tables -> pinned staging copy k."""
        dst, tab, extra = plan["pinned"][k].numpy(), plan["tab"], plan["extra"]
        dst[:tab.nbytes] = tab.view(np.uint8).reshape(-1)
        if extra is not None:
            dst[tab.nbytes:] = extra.view(np.uint8).reshape(-1)

    @staticmethod
    def _extra_ptr(plan):
        return plan["dev_tab"].data_ptr() + plan["tab"].nbytes          # (64-byte rows in front: 16-byte aligned)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError(self._SPARSE_MESSAGE)
                if not p.is_cuda:
                    raise RuntimeError("vilbert.optim.%s runs on HIP devices only - no CPU fallback" % self._NAME)
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise RuntimeError("vilbert.optim.%s needs contiguous fp32 parameters" % self._NAME)
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p)
                    state["exp_avg_sq"] = torch.zeros_like(p)
                state["step"] += 1
                entries.append((p, state, group))
        if not entries:
            return loss
        self._ensure_arena()
        device = entries[0][0].device
        key = tuple((p.data_ptr(), st["exp_avg"].data_ptr()) for p, st, _ in entries)
        if key != self._plan_key:
            self._plan_key, self._plan = key, self._build_plan(entries, device)
        plan = self._plan
        capturing = torch.cuda.is_current_stream_capturing()
        keep = self._fill_table(plan, entries)
        # asynchronous upload through pinned memory: no host <-> device synchronisation in step()
        if capturing:
            # HIP-graph capture: the copy node reads pinned buffer 0 at every replay; prepare_replay() refreshes it
            k = 0
            self._captured = (plan, entries)
        else:
            k = plan["turn"]
            plan["turn"] = k ^ 1
            if plan["events"][k] is not None:
                plan["events"][k].synchronize()
        self._stage(plan, k)
        dev_tab = plan["dev_tab"]
        dev_tab.copy_(plan["pinned"][k], non_blocking=True)
        if not capturing:
            ev = torch.cuda.Event()
            ev.record()
            plan["events"][k] = ev
        if self._scaled():
            partials, state = self._clip_buffers(plan, device)
            skip = int(self.skip_nonfinite)
            N.check(N.lib().vbx_grad_norm(*self._table_args(plan), self.max_grad_norm, self.grad_scale, skip,
                                          partials.data_ptr(), state.data_ptr()), "vbx_grad_norm")
            self._launch(plan, state, skip)
        else:
            self._launch(plan, None, 0)
        N.weights_changed()
        del keep
        return loss

    @classmethod
    def _table_args(cls, plan, scalars=False):
        """The leading arguments of every native entry point: stream, chunk count, tensor table (`scalars`: the class's
        second table right behind it), chunk lists, chunk size."""
        tables = (plan["dev_tab"].data_ptr(),) + ((cls._extra_ptr(plan),) if scalars else ())
        return (N.stream_ptr(), plan["n_chunks"]) + tables + (plan["chunk_tensor"].data_ptr(), plan["chunk_off"].data_ptr(),
                                                             CHUNK_ELEMS)

    def _scaled(self):
        return self.max_grad_norm > 0.0 or self.grad_scale != 1.0 or self.skip_nonfinite

    def _allocating(self, step, buffers):
        """Fixed-address device buffers are allocated by the first eager step that needs them - never inside a capture."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("%s: the first %s of a plan allocates its %s and must run eagerly before a graph capture "
                               "(GraphedTrainStep's warm-up does)" % (self._NAME, step, buffers))

    def _clip_buffers(self, plan, device):
        """Fixed-address buffers of the norm pass: the per-chunk partial sums belong to the plan, the state (norm,
        coefficient, finite flag, skipped-step count) to the optimizer - the count survives a change of plan."""
        if self._grad_state is None or "partials" not in plan:
            self._allocating("clipped / scaled step", "buffers")
            if self._grad_state is None:
                self._grad_state = torch.zeros(N.GRAD_STATE_FLOATS, dtype=torch.float32, device=device)
            plan["partials"] = torch.empty(int(N.lib().vbx_grad_norm_workspace(plan["n_chunks"])), dtype=torch.float32,
                                           device=device)
        return plan["partials"], self._grad_state

    def _need_state(self):
        if self._grad_state is None:
            raise RuntimeError(self._NAME + ": no clipped / scaled step has run yet (max_grad_norm, grad_scale and skip_nonfinite "
                               "are all at their defaults, or step() was never called)")
        return self._grad_state

    @property
    def grad_norm(self):
        """Global norm of the (scaled) gradients of the last clipped / scaled step: a 0-dim DEVICE tensor that views the
        state the norm kernel writes - reading the property does not synchronise, and the same tensor shows the value of
        every later step (also of graph replays). Clone it to keep a value."""
        return self._need_state()[N.GRAD_STATE_NORM]

    def skipped_steps(self):
        """Number of steps skipped because of non-finite gradients (skip_nonfinite=True). Reads the device counter:
        SYNCHRONISES with the device."""
        return 0 if self._grad_state is None else int(self._grad_state[N.GRAD_STATE_SKIPPED].item())

    def last_step_skipped(self):
        """Whether the last step was skipped (skip_nonfinite=True and non-finite gradients). SYNCHRONISES with the device."""
        if not self.skip_nonfinite or self._grad_state is None:
            return False
        return float(self._grad_state[N.GRAD_STATE_FINITE].item()) == 0.0

    def _fill_table(self, plan, entries, pointers=True):
        """Per-step columns of the launch table: gradient pointers and the hyper-parameters of this step."""
        tab = plan["tab"]
        keep = []
        if pointers:
            for i, (p, st, g) in enumerate(entries):
                grad = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                keep.append(grad)
                tab["grad"][i] = grad.data_ptr()
        self._fill_hyper(plan, entries)
        return keep

    def _group_index(self, plan, entries):
        """Index of every entry's parameter group (cached in the plan)."""
        gi = plan.get("group_index")
        if gi is None or len(gi) != len(entries):
            ids = {id(g): k for k, g in enumerate(self.param_groups)}
            gi = plan["group_index"] = np.array([ids[id(g)] for _p, _st, g in entries], dtype=np.int64)
        return gi

    def _hyper_columns(self, plan, entries, *switches):
        """One float64 value per entry of lr, beta1, beta2, eps, weight_decay (through the group index) and of the tensor's
        own step count, then one boolean per entry for every group key in `switches`. (vectorised: this runs on the host
        once per step, ~530 rows)"""
        gi = self._group_index(plan, entries)
        groups = self.param_groups
        cols = [[g["lr"] for g in groups], [g["betas"][0] for g in groups], [g["betas"][1] for g in groups],
                [g["eps"] for g in groups], [g["weight_decay"] for g in groups]]
        cols = [np.array(c, dtype=np.float64)[gi] for c in cols]
        cols.append(np.fromiter((st["step"] for _p, st, _g in entries), dtype=np.float64, count=len(entries)))
        return cols + [np.array([bool(g[k]) for g in groups])[gi] for k in switches]

    def prepare_replay(self):
        """Host side of one replay of a captured step (GraphedTrainStep): advances the step counts and rewrites the
        pinned table the captured copy node reads (learning-rate schedule, bias correction). The previous replay
        must have finished reading the table (the caller synchronises)."""
        plan, entries = self._captured
        for _p, st, _g in entries:
            st["step"] += 1
        self._fill_table(plan, entries, pointers=False)     # the gradients live at fixed addresses (arena)
        self._stage(plan, 0)


class AdamW(_MultiTensorOptimizer):
    """Adam with decoupled weight decay; ``correct_bias=False`` reproduces the original BERT optimizer
    (train_tasks.py:426). State layout (``step``, ``exp_avg``, ``exp_avg_sq``) matches pytorch-transformers, so
    the ``.tar`` checkpoints the reference scripts write stay interchangeable.

    ``max_grad_norm``, ``grad_scale`` and ``skip_nonfinite`` are those of the base class. That ``state["step"]`` advances
    on the host also for a skipped step only matters with ``correct_bias=True``, which neither reference script uses."""

    _NAME = "AdamW"
    _SPARSE_MESSAGE = "Adam does not support sparse gradients, please consider SparseAdam instead"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, correct_bias=True,
                 max_grad_norm=0.0, grad_scale=1.0, skip_nonfinite=False):
        _check_adam_args(lr, betas, eps)
        self._init_native(max_grad_norm, grad_scale, skip_nonfinite)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, correct_bias=correct_bias)
        super(AdamW, self).__init__(params, defaults)
        self._init_plan()

    def _fill_hyper(self, plan, entries):
        tab = plan["tab"]
        lr, b1, b2, eps, wd, steps, corr = self._hyper_columns(plan, entries, "correct_bias")
        step_size = np.where(corr, lr * np.sqrt(1.0 - b2 ** steps) / (1.0 - b1 ** steps), lr)
        tab["step_size"], tab["beta1"], tab["beta2"] = step_size, b1, b2
        tab["eps"], tab["decay"] = eps, lr * wd

    def _launch(self, plan, state, skip):
        args = self._table_args(plan)
        if state is None:
            N.check(N.lib().vb_adamw_step(*args), "vb_adamw_step")
        else:
            N.check(N.lib().vbx_adamw_step_scaled(*(args + (state.data_ptr(), skip))), "vbx_adamw_step_scaled")


def radam_schedule(step, lr, beta1, beta2):
    """Host side of one RAdam step for a tensor at 1-based `step`, in double: (N_sma, step_size). N_sma is the length of
    the approximated simple moving average (rho_t of the paper); from N_sma >= 5 on the step is rectified - the adaptive
    update scaled by r_t = sqrt((N-4)(N-2) N_max / ((N_max-4)(N_max-2) N)) and by the bias correction of the second
    moment - before that it is SGD with (bias-corrected) momentum. The products and quotients run left to right in the
    reference's order, so that the doubles agree to the bit."""
    beta2_t = beta2 ** step
    n_max = 2 / (1 - beta2) - 1
    n_sma = n_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma >= 5:
        rect = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max / (n_max - 2))
        return n_sma, lr * rect / (1 - beta1 ** step)
    return n_sma, lr / (1 - beta1 ** step)


class PlainRAdam(_MultiTensorOptimizer):
    """Rectified Adam with the constructor, the arithmetic and the state layout (``step``, ``exp_avg``, ``exp_avg_sq``) of
    the reference's ``vilbert.optimization.PlainRAdam``, as ONE native multi-tensor launch (csrc/optimizer.hip:
    radam_kernel). Checkpoints are interchangeable with the reference class in both directions. Every tensor's step size
    comes from its own step count and its own group's learning rate. Parameters without a gradient are skipped and their
    step count does not advance. ``max_grad_norm`` / ``grad_scale`` / ``skip_nonfinite`` as in the base class (the
    reference classes have none of the three; the defaults leave them off)."""

    _NAME = "PlainRAdam"
    _SPARSE_MESSAGE = "RAdam does not support sparse gradients"
    _EXTRA_DTYPE = _RADAM_DTYPE

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 max_grad_norm=0.0, grad_scale=1.0, skip_nonfinite=False):
        self._init_native(max_grad_norm, grad_scale, skip_nonfinite)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super(PlainRAdam, self).__init__(params, defaults)
        self._init_plan()

    def _schedule(self, step, group):
        beta1, beta2 = group["betas"]
        return radam_schedule(step, group["lr"], beta1, beta2)

    def _fill_hyper(self, plan, entries):
        """One pass in parameter-group order (RAdam's step-size cache depends on that order); the arithmetic is Python
        floats, i.e. double."""
        assert ctypes.sizeof(N.RAdamScalars) == _RADAM_DTYPE.itemsize
        n = len(entries)
        cols = np.empty((7, n), dtype=np.float64)
        rect = np.empty(n, dtype=np.int32)
        for i, (_p, st, group) in enumerate(entries):
            n_sma, step_size = self._schedule(st["step"], group)
            beta1, beta2 = group["betas"]
            cols[:, i] = (step_size, group["weight_decay"] * group["lr"], beta1, beta2, 1 - beta1, 1 - beta2, group["eps"])
            rect[i] = n_sma >= 5
        extra = plan["extra"]
        for k, name in enumerate(("step_size", "decay", "beta1", "beta2", "one_minus_beta1", "one_minus_beta2", "eps")):
            extra[name] = cols[k]
        extra["rectified"] = rect

    def _launch(self, plan, state, skip):
        N.check(N.lib().vbo_radam_step(*self._table_args(plan, scalars=True), None if state is None else state.data_ptr(),
                                       skip), "vbo_radam_step")


class RAdam(PlainRAdam):
    """The reference's ``vilbert.optimization.RAdam`` (``train_tasks.py --optim RAdam``) on the native launch. It differs
    from PlainRAdam in one deliberate quirk, reproduced here because it decides real trajectories: ``self.buffer`` caches
    ``[step, N_sma, step_size]`` in ten slots indexed by ``step % 10``, and the cached ``step_size`` already contains the
    learning rate. Whichever tensor reaches a step count first fills the slot with ITS group's lr, and every later tensor
    at the same step count - in this step() call or a later one - takes that step size whatever its own group's lr is.
    train_tasks.py builds one group per parameter with task-dependent learning rates, so all of them move with the step
    size of the first group. Weight decay is not cached: it uses each group's own ``lr * weight_decay``. The buffer is
    not part of ``state_dict()`` (nor is it upstream): after a reload it refills on the next step."""

    _NAME = "RAdam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 max_grad_norm=0.0, grad_scale=1.0, skip_nonfinite=False):
        self.buffer = [[None, None, None] for _ in range(10)]
        super(RAdam, self).__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                    max_grad_norm=max_grad_norm, grad_scale=grad_scale, skip_nonfinite=skip_nonfinite)

    def __setstate__(self, state):
        super(RAdam, self).__setstate__(state)
        if not hasattr(self, "buffer"):
            self.buffer = [[None, None, None] for _ in range(10)]

    def _schedule(self, step, group):
        slot = self.buffer[int(step % 10)]
        if step != slot[0]:
            slot[0] = step
            slot[1], slot[2] = super(RAdam, self)._schedule(step, group)
        return slot[1], slot[2]


# The classes carry the module path they have upstream, `vilbert.optimization` - the path the scripts import them from and
# the one a whole-object pickle (`torch.save(optimizer)`) records, so that such a pickle written upstream resolves to the
# native class here and vice versa (vilbert/utils.py does the same for the reference's logging classes). The finder in
# vilbert/__init__.py makes `vilbert.optimization.RAdam` this very class.
RAdam.__module__ = PlainRAdam.__module__ = "vilbert.optimization"


class LAMB(_MultiTensorOptimizer):
    """LAMB (You et al. 2020, "Large Batch Optimization for Deep Learning: Training BERT in 76 minutes"): Adam with one trust
    ratio ||p|| / ||update|| per parameter tensor, the optimizer BERT pre-training uses at global batches of thousands of
    samples. Two native launches after the optional norm pass (csrc/lamb.hip, include/vilbert_hip_lamb.h). Per tensor, in
    fp32 on the device, with g the gradient times the base class's clip / scale coefficient:

        L2 mode (adam_w_mode=False):  g += weight_decay * p
        m = beta1 * m + beta3 * g             beta3 = 1 - beta1 with grad_averaging, else 1
        v = beta2 * v + (1 - beta2) * g * g
        u = (m / bc1) / (sqrt(v / bc2) + eps)  [+ weight_decay * p  with adam_w_mode]
                                              bc = 1 - beta^t with bias_correction, else 1; t = the tensor's own 1-based step count
        r = ||p|| / ||u||  if (use_nvlamb or weight_decay != 0) and ||p|| > 0 and ||u|| > 0, else 1
        p = p - lr * r * u

    ``lr``, ``betas``, ``eps``, ``weight_decay``, ``bias_correction`` and ``grad_averaging`` are per parameter group;
    ``adam_w_mode`` and ``use_nvlamb`` hold for the whole optimizer. The scalars of a step are computed on the host in double
    and rounded once to float. State layout (``step``, ``exp_avg``, ``exp_avg_sq``) as the other classes of this module.
    ``max_grad_norm`` (default 1.0, as LAMB is usually run), ``grad_scale`` and ``skip_nonfinite`` are those of the base
    class; a skipped step leaves parameters, moments and ``trust_ratios`` untouched. The norms are summed without atomics in a
    fixed order: the same inputs give the same bits, wherever a tensor stands in the parameter list. Unlike the other classes
    a pickled LAMB keeps its optimizer-wide settings."""

    _NAME = "LAMB"
    _SPARSE_MESSAGE = "LAMB does not support sparse gradients"
    _EXTRA_DTYPE = _LAMB_DTYPE
    _PICKLED = ("adam_w_mode", "use_nvlamb", "max_grad_norm", "grad_scale", "skip_nonfinite")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, bias_correction=True,
                 grad_averaging=True, adam_w_mode=True, use_nvlamb=False, max_grad_norm=1.0, grad_scale=1.0,
                 skip_nonfinite=False):
        _check_adam_args(lr, betas, eps)
        self._init_native(max_grad_norm, grad_scale, skip_nonfinite)
        self.adam_w_mode, self.use_nvlamb = bool(adam_w_mode), bool(use_nvlamb)
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, bias_correction=bool(bias_correction),
                        grad_averaging=bool(grad_averaging))
        super(LAMB, self).__init__(params, defaults)
        self._init_plan()

    def __getstate__(self):
        state = dict(super(LAMB, self).__getstate__())
        state.update((k, getattr(self, k)) for k in self._PICKLED)
        return state

    def __setstate__(self, state):
        super(LAMB, self).__setstate__(state)          # (the base class puts the clipping attributes back at ITS defaults)
        for k in self._PICKLED:
            if k in state:
                setattr(self, k, state[k])

    def _fill_hyper(self, plan, entries):
        """(a tensor's chunks are consecutive in the chunk list, so its first chunk is the number of chunks in front of it)"""
        assert ctypes.sizeof(N.LambScalars) == _LAMB_DTYPE.itemsize
        extra = plan["extra"]
        lr, b1, b2, eps, wd, steps, corr, avg = self._hyper_columns(plan, entries, "bias_correction", "grad_averaging")
        extra["lr"], extra["weight_decay"], extra["beta1"], extra["beta2"], extra["eps"] = lr, wd, b1, b2, eps
        extra["beta3"] = np.where(avg, 1.0 - b1, 1.0)
        extra["one_minus_beta2"] = 1.0 - b2
        extra["bc1"] = np.where(corr, 1.0 - b1 ** steps, 1.0)
        extra["bc2"] = np.where(corr, 1.0 - b2 ** steps, 1.0)
        extra["adam_w_mode"] = int(self.adam_w_mode)
        extra["apply_trust"] = (wd != 0.0) | self.use_nvlamb
        if "lamb_index" not in plan:
            counts = -(-plan["tab"]["numel"] // CHUNK_ELEMS)
            plan["lamb_chunks"] = (np.cumsum(counts) - counts, counts)
            plan["lamb_index"] = {id(p): i for i, (p, _st, _g) in enumerate(entries)}
        extra["first_chunk"], extra["n_chunks"] = plan["lamb_chunks"]

    def _lamb_buffers(self, plan):
        """Fixed-address buffers of the two stages, both the plan's: the per-chunk partial sums of p^2 and u^2 and the
        per-tensor trust ratios (1 until a step has run)."""
        if "trust" not in plan:
            self._allocating("step", "trust-ratio buffers")
            device = plan["dev_tab"].device
            plan["lamb_workspace"] = torch.empty(int(N.lib().vbl_lamb_workspace(plan["n_chunks"])), dtype=torch.float32,
                                                 device=device)
            plan["trust"] = torch.ones(len(plan["tab"]), dtype=torch.float32, device=device)
        return plan["lamb_workspace"], plan["trust"]

    def _launch(self, plan, state, skip):
        workspace, trust = self._lamb_buffers(plan)
        N.check(N.lib().vbl_lamb_step(*self._table_args(plan, scalars=True), workspace.data_ptr(), trust.data_ptr(),
                                      None if state is None else state.data_ptr(), skip), "vbl_lamb_step")

    def _need_trust(self):
        if self._plan is None or "trust" not in self._plan:
            raise RuntimeError(self._NAME + ": no step has run yet - there are no trust ratios")
        return self._plan

    @property
    def trust_ratios(self):
        """The trust ratio r of every tensor the last step updated, in the order the step walked them (parameter groups in
        order, parameters without a gradient left out): a DEVICE tensor the update kernel writes - reading the property does
        not synchronise, and the same tensor shows the values of every later step with the same set of tensors (also of
        graph replays). Clone it to keep the values."""
        return self._need_trust()["trust"]

    def trust_ratio(self, p):
        """The 0-dim device view of `trust_ratios` for parameter `p`."""
        plan = self._need_trust()
        i = plan["lamb_index"].get(id(p))
        if i is None:
            raise KeyError(self._NAME + ": the last step did not update this tensor (no gradient, or not a parameter of this "
                           "optimizer)")
        return plan["trust"][i]


class ConstantLRSchedule(LambdaLR):
    def __init__(self, optimizer, last_epoch=-1):
        super(ConstantLRSchedule, self).__init__(optimizer, lambda _: 1.0, last_epoch=last_epoch)


class WarmupConstantSchedule(LambdaLR):
    """Linear warm-up 0 -> 1 over ``warmup_steps`` steps, then constant (train_tasks.py:437)."""

    def __init__(self, optimizer, warmup_steps, last_epoch=-1):
        self.warmup_steps = warmup_steps
        super(WarmupConstantSchedule, self).__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1.0, self.warmup_steps))
        return 1.0


class WarmupLinearSchedule(LambdaLR):
    """Linear warm-up 0 -> 1 over ``warmup_steps``, then linear decay to 0 at ``t_total``
    (train_concap.py:472-476, train_tasks.py:433-435)."""

    def __init__(self, optimizer, warmup_steps, t_total, last_epoch=-1):
        self.warmup_steps, self.t_total = warmup_steps, t_total
        super(WarmupLinearSchedule, self).__init__(optimizer, self.lr_lambda, last_epoch=last_epoch)

    def lr_lambda(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1, self.warmup_steps))
        return max(0.0, float(self.t_total - step) / float(max(1.0, self.t_total - self.warmup_steps)))
