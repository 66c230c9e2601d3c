"""Run the reference's own batch-finishing code without importing its module (tensorpack / lmdb / boto3
are not installed): the function source is cut out of the reference file with ``ast`` and compiled as it
stands. Build container only - /root/reference does not exist on the GPU box."""
import ast
import os

import numpy as np
import torch

from oracle.ref_loader import REFERENCE_ROOT as REF  # (VILBERT_REFERENCE_ROOT, as for the model)


def available():
    return os.path.isfile(os.path.join(REF, "vilbert", "datasets", "concept_cap_dataset.py"))


def _source_of(path, pick):
    text = open(path, encoding="utf-8").read()
    tree = ast.parse(text)
    node = pick(tree)
    return ast.get_source_segment(text, node), node


def reference_loader_iter(raw_tuple_batches):
    """ConceptCapLoaderTrain.__iter__ (concept_cap_dataset.py:241-282) run over the given raw batches."""
    def pick(tree):
        for cls in tree.body:
            if isinstance(cls, ast.ClassDef) and cls.name == "ConceptCapLoaderTrain":
                for fn in cls.body:
                    if isinstance(fn, ast.FunctionDef) and fn.name == "__iter__":
                        return fn
        raise LookupError("ConceptCapLoaderTrain.__iter__")
    src, _ = _source_of(os.path.join(REF, "vilbert", "datasets", "concept_cap_dataset.py"), pick)
    ns = {"np": np, "torch": torch}
    import textwrap
    exec(compile(textwrap.dedent(src), "<reference ConceptCapLoaderTrain.__iter__>", "exec"), ns)

    class _DS(object):
        def get_data(self):
            return iter(raw_tuple_batches)

    class _Self(object):
        ds = _DS()
    return list(ns["__iter__"](_Self()))


def reference_objective1_edit(image_label, lm_label_ids, is_next):
    """The `if args.objective == 1:` block of the training loop (train_concap.py:535-540) on torch tensors."""
    def pick(tree):
        for node in ast.walk(tree):
            if isinstance(node, ast.If) and isinstance(node.test, ast.Compare):
                seg = ast.dump(node.test)
                if "objective" in seg and any(isinstance(s, ast.Assign) and getattr(s.targets[0], "id", "") == "image_label"
                                              for s in node.body):
                    return node
        raise LookupError("objective == 1 block")
    src, _ = _source_of(os.path.join(REF, "train_concap.py"), pick)
    import textwrap

    class _Args(object):
        objective = 1
    ns = {"args": _Args(), "image_label": image_label.clone(), "lm_label_ids": lm_label_ids.clone(),
          "is_next": is_next.clone(), "torch": torch}
    exec(compile(textwrap.dedent(src), "<reference train_concap objective-1 block>", "exec"), ns)
    return ns["image_label"], ns["lm_label_ids"]
