"""What ``import vilbert.optimization`` gives when NO reference checkout is attached (vilbert/__init__.py:
_OptimizationFinder): the two names the fine-tuning script takes from that module (``from vilbert.optimization import RAdam``,
train_tasks.py:32,427-428), as the native classes of ``vilbert.optim`` (csrc/optimizer.hip: radam_kernel). With a checkout
attached the module is the reference's own file with these two names rebound to the same classes, and this file is not used.
"""
from .optim import PlainRAdam, RAdam

__all__ = ["RAdam", "PlainRAdam"]


def __getattr__(name):
    raise AttributeError("vilbert.optimization.%s: this package provides RAdam and PlainRAdam; every other name is the "
                         "reference's, and no reference checkout is attached (set VILBERT_REFERENCE_ROOT)" % name)
