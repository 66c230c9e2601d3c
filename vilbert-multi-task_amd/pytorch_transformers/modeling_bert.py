"""Import-name shim: the reference's `--baseline` switch (train_tasks.py:181-183, eval_tasks.py:136-138) imports
``from pytorch_transformers.modeling_bert import BertConfig`` for its single-stream baseline model
(vilbert/basebert.py - native here too: BaseBertForVLTasks and BertModel accept this config, or any object with the same
attributes). The name resolves to `transformers.BertConfig` when installed."""
from transformers import BertConfig  # noqa: F401
