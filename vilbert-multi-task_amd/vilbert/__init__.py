"""MI355X-native ``vilbert`` package: import-compatible with the reference's ``vilbert`` for the model
path (``from vilbert.vilbert import BertConfig, BertForMultiModalPreTraining, VILBertForVLTasks``)."""

import os as _os

# A training step keeps up to four HIP streams busy (text | image encoder streams, each with a weight-gradient side
# stream - autograd_ops.py), plus RCCL's own in data-parallel runs. HIP maps streams round-robin onto
# GPU_MAX_HW_QUEUES (default 4) hardware queues; streams that share a queue serialise and the overlap silently
# disappears (measured, B = 256 step: 2,375 samples/s with 4 queues, 2,422-2,429 with 6-8; B = 64: 1,887 -> 1,913).
# The variable is read when the HIP runtime initialises, i.e. at the first device call - importing this package early
# (the training scripts do) is in time. (A whole-step HIP graph replays faster with 4 queues: vilbert/graphed.py.)
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


# --- fall-through to the reference checkout for everything that is NOT the hot path -----------------------------
# This package replaces `vilbert.vilbert` (the model) and `vilbert.utils.PreTrainedModel`; the reference's training
# scripts also import `vilbert.datasets`, `vilbert.task_utils`, `vilbert.optimization`, `vilbert.basebert`
# (train_concap.py:29-31, train_tasks.py:32-46) - data / control side, not rebuilt here. A regular package named
# `vilbert` would hide those, so the reference's own `vilbert/` directory is appended to `__path__` AFTER ours:
# submodules that exist here resolve here, every other one is the reference's file, unmodified.
def _reference_package_dir():
    """The reference checkout's `vilbert/` directory: $VILBERT_REFERENCE_ROOT, else the first sys.path entry / the
    working directory that holds a foreign `vilbert/task_utils.py` (the scripts are run from their checkout)."""
    import sys
    here = _os.path.dirname(_os.path.abspath(__file__))
    roots = [_os.environ["VILBERT_REFERENCE_ROOT"]] if _os.environ.get("VILBERT_REFERENCE_ROOT") else \
        [p or _os.getcwd() for p in sys.path] + [_os.getcwd()]
    for root in roots:
        cand = _os.path.join(_os.path.abspath(root), "vilbert")
        if cand != here and _os.path.isfile(_os.path.join(cand, "task_utils.py")):
            return cand
    return None


def attach_reference(root=None):
    """(Re)run the search - `root` overrides it - and append the reference's package directory to `__path__`.
    Returns the directory or None. Idempotent; called once at import."""
    global REFERENCE_PACKAGE_DIR
    cand = _os.path.join(_os.path.abspath(root), "vilbert") if root else _reference_package_dir()
    if cand and _os.path.isdir(cand):
        if cand not in __path__:
            __path__.append(cand)
        REFERENCE_PACKAGE_DIR = cand
    return REFERENCE_PACKAGE_DIR


REFERENCE_PACKAGE_DIR = None
attach_reference()


# --- `vilbert.optimization`: the reference's module, with RAdam / PlainRAdam on the native step -----------------------
# train_tasks.py:32 does `from vilbert.optimization import RAdam` (`--optim RAdam`). The module stays what the fall-through
# makes it - the reference's own file, every name of it as upstream - except that its two optimizer classes are rebound to
# the native ones (vilbert/optim.py: one multi-tensor launch per step instead of a Python loop over ~400 tensors). A file
# `optimization.py` in this directory would hide the reference's module altogether, so the rebinding is done by a finder
# for this one name; without a checkout (the GPU-only install) the name resolves to vilbert/_optimization.py, which offers
# the two classes alone. Lazy: nothing is imported until somebody asks for the module.
class _RebindingLoader(object):
    """The loader the path search found, plus the assignments (`rebind(module)`) after the module body ran."""

    def __init__(self, inner, rebind):
        self._inner = inner
        self._rebind = rebind

    def __getattr__(self, name):          # get_source, get_code, is_package, ...: the inner loader's
        return getattr(self._inner, name)

    def create_module(self, spec):
        return self._inner.create_module(spec)

    def exec_module(self, module):
        self._inner.exec_module(module)
        self._rebind(module)


def _rebind_optimization(module):
    from . import optim
    module.RAdam, module.PlainRAdam = optim.RAdam, optim.PlainRAdam


# --- `vilbert.task_utils`: the reference's module, with its criteria and answer score on the native kernels ----------
# train_tasks.py:41-46 takes LoadLosses / ForwardModelsTrain / ForwardModelsVal from it; those read the module globals
# `LossMap` (the criterion objects, task_utils.py:25-28) and `compute_score_with_logits` (:618-623) at call time. The same
# finder serves this name: the module is the reference's own file - `__file__` and every other name of it as upstream -
# and after its body ran the two LossMap entries are instances of vilbert/task_losses.py's subclasses of the same torch
# modules (native on fp32 HIP tensors, `super().forward` everywhere else) and the score function is task_losses'. There
# is no stand-in: without a checkout the name stays unimportable, as the rest of the reference's data side does.
def _rebind_task_utils(module):
    from . import task_losses
    module.LossMap["BCEWithLogitLoss"] = task_losses.BCEWithLogitsLoss(reduction="mean")
    module.LossMap["CrossEntropyLoss"] = task_losses.CrossEntropyLoss()
    module.compute_score_with_logits = task_losses.compute_score_with_logits
    # one added name: which output of VILBertForVLTasks each task type reads (for model.set_active_heads)
    module.HEAD_OF_TASK_TYPE = task_losses.HEAD_OF_TASK_TYPE


class _OptimizationFinder(object):
    @staticmethod
    def find_spec(fullname, path=None, target=None):
        if fullname not in (__name__ + ".optimization", __name__ + ".task_utils"):
            return None
        from importlib.machinery import PathFinder
        from importlib.util import spec_from_file_location
        spec = PathFinder.find_spec(fullname, list(__path__))          # the reference's file, if a checkout is attached
        if fullname == __name__ + ".task_utils":
            if spec is None or spec.loader is None:
                return None                                             # no checkout: the ordinary search fails as it always did
            spec.loader = _RebindingLoader(spec.loader, _rebind_task_utils)
            return spec
        if spec is None or spec.loader is None:
            spec = spec_from_file_location(fullname, _os.path.join(_os.path.dirname(_os.path.abspath(__file__)),
                                                                   "_optimization.py"))
        spec.loader = _RebindingLoader(spec.loader, _rebind_optimization)
        return spec


def _install_optimization_finder():
    import sys
    if not any(isinstance(f, type) and f.__name__ == "_OptimizationFinder" for f in sys.meta_path):
        sys.meta_path.insert(0, _OptimizationFinder)


_install_optimization_finder()


# --- the device-side batch builder of the fine-tuning tasks, by name ----------------------------------------------------
# `from vilbert import TaskBatchPipeline` (vilbert/task_pipeline.py). Resolved on first use: importing the package loads
# neither torch nor the native library.
_TASK_PIPELINE_NAMES = ("raw_item", "pack_task_samples", "finish_task_batch", "dense_target", "TaskBatchPipeline")
# `from vilbert import RegionStore` (vilbert/region_store.py): the device-resident region store and its pipeline
_REGION_STORE_NAMES = ("RegionStore", "StoreBatchPipeline")


def __getattr__(name):
    if name in _TASK_PIPELINE_NAMES:
        from . import task_pipeline
        return getattr(task_pipeline, name)
    if name in _REGION_STORE_NAMES:
        from . import region_store
        return getattr(region_store, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
