"""Single-stream baseline model for MI355X - drop-in for the reference's ``vilbert.basebert`` (``--baseline``).

Text tokens and image regions are embedded into ONE ``[B, T + R, H]`` sequence that runs through a plain BERT encoder (the
VisualBERT / UNITER shape). Same public classes, constructor / forward signatures, ``state_dict`` names and output order as
the reference's file (cited per class), every forward enqueues the gfx950 kernels of libvilbert_hip.so:

* both embeddings, their two LayerNorms and the additive attention mask of the two masks are one launch that writes the joint
  buffer directly (csrc/joint_embed.hip) - no ``torch.cat`` of the states or of the masks;
* an encoder layer is exactly ``vilbert.vilbert.BertLayer`` (one call across the C ABI per layer);
* the pooler is the GEMM on the first-token rows (read in place through the row stride) followed by a tanh kernel;
* the heads are the GEMMs / LayerNorms of the two-stream heads.

``nn.Linear`` / ``nn.Embedding`` / ``nn.Dropout`` children exist so that parameter names, shapes and registration order are
the reference's; their own ``forward`` is never used. fp32 only: ``half()`` and a forward under the process-wide bf16 / fp8 /
MX modes raise ``NotImplementedError`` (the fp32-tensor GEMM modes bf16x6 / bf16x3 live inside the GEMM and just work). There
is no CPU path.

Not driven by the reference's multi-task trainer: ``ForwardModelsTrain`` / ``ForwardModelsVal`` unpack ten outputs and pass
``task_tokens``, the reference's own ``BaseBertForVLTasks`` returns seven and takes no task ids - the class API below is the
reference's.
"""
import logging
import os
import types

import torch
from torch import nn
from torch.nn import CrossEntropyLoss
from torch.nn.utils.weight_norm import weight_norm

from . import _native
from . import functional as F
from . import ops
from .vilbert import (BertLayer, BertLayerNorm, BertLMPredictionHead, BertPredictionHeadTransform, _act_name, _check_head_dim,
                      _drop_p, _dropout, _skip_dropout_seed)

logger = logging.getLogger(__name__)

WEIGHTS_NAME = "pytorch_model.bin"
IMAGE_FEATURE_SIZE = 2048       # reference basebert.py:330
IMAGE_TARGET_SIZE = 1601        # reference basebert.py:629

# The seven outputs of BaseBertForVLTasks.forward, in the order of the returned tuple (reference basebert.py:954-962)
BASEBERT_HEADS = ("vil_prediction", "vil_logit", "vil_binary_prediction", "vision_prediction", "vision_logit",
                  "linguisic_prediction", "linguisic_logit")


def _require_fp32_stream(what):
    if _native.bf16_stream() or _native.fp8_enabled() or _native.mx_enabled():
        raise NotImplementedError("%s runs on the fp32 stream only: the process-wide bf16 / fp8 / MX GEMM mode is on "
                                  "(_native.set_gemm_mode); use \"f32\", \"bf16x6\" or \"bf16x3\"" % what)


def _layer_config(config):
    """What vilbert.vilbert.BertLayer reads, taken from any config object (transformers.BertConfig, vilbert.vilbert.BertConfig, a
    namespace); the baseline has no attention-map output."""
    return types.SimpleNamespace(
        hidden_size=config.hidden_size, num_attention_heads=config.num_attention_heads,
        intermediate_size=config.intermediate_size, hidden_act=_act_name(config.hidden_act),
        hidden_dropout_prob=config.hidden_dropout_prob, attention_probs_dropout_prob=config.attention_probs_dropout_prob,
        visualization=False)


class BertPreTrainedModel(nn.Module):
    """Weight initialisation and checkpoint loading, reference basebert.py:85-281. Any object carrying the attributes read is
    accepted as config."""

    def __init__(self, config, *inputs, **kwargs):
        super(BertPreTrainedModel, self).__init__()
        self.config = config

    def init_bert_weights(self, module):
        if isinstance(module, (nn.Linear, nn.Embedding)):
            module.weight.data.normal_(mean=0.0, std=self.config.initializer_range)
        elif isinstance(module, BertLayerNorm):
            module.bias.data.zero_()
            module.weight.data.fill_(1.0)
        if isinstance(module, nn.Linear) and module.bias is not None:
            module.bias.data.zero_()

    def half(self):
        raise NotImplementedError("vilbert.basebert: the baseline model runs on the fp32 stream only (no bf16 / fp16 execution)")

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, config, state_dict=None, cache_dir=None, from_tf=False,
                        *inputs, **kwargs):
        """Local files only: a directory holding ``pytorch_model.bin``, a ``.bin`` file, or ``state_dict=``. The reference's two
        key rules apply: ``gamma`` -> ``weight`` / ``beta`` -> ``bias``, and a checkpoint with ``bert.``-prefixed keys loads
        into a model that has no ``bert`` child (:219-262). Returns None when the file does not exist, as the reference does."""
        if from_tf:
            raise NotImplementedError("TensorFlow checkpoints are not supported by this build")
        if state_dict is None:
            path = pretrained_model_name_or_path
            weights = os.path.join(path, WEIGHTS_NAME) if os.path.isdir(path) else path
            if not os.path.isfile(weights):
                logger.error("Model name '%s' was not found; assumed '%s' was a path but no file is there.", path, weights)
                return None
            state_dict = torch.load(weights, map_location="cpu")
        model = cls(config, *inputs, **kwargs)
        metadata = getattr(state_dict, "_metadata", None)
        renamed = {}
        for key, value in state_dict.items():
            renamed[key.replace("gamma", "weight").replace("beta", "bias")] = value
        missing_keys, unexpected_keys, error_msgs = [], [], []

        def load(module, prefix=""):
            local_metadata = {} if metadata is None else metadata.get(prefix[:-1], {})
            module._load_from_state_dict(renamed, prefix, local_metadata, True, missing_keys, unexpected_keys, error_msgs)
            for name, child in module._modules.items():
                if child is not None:
                    load(child, prefix + name + ".")

        start_prefix = ""
        if not hasattr(model, "bert") and any(s.startswith("bert.") for s in renamed):
            start_prefix = "bert."
        load(model, prefix=start_prefix)
        if missing_keys:
            logger.info("Weights of %s not initialized from pretrained model: %s", model.__class__.__name__, missing_keys)
        if unexpected_keys:
            logger.info("Weights from pretrained model not used in %s: %s", model.__class__.__name__, unexpected_keys)
        if error_msgs:
            raise RuntimeError("Error(s) in loading state_dict for {}:\n\t{}".format(model.__class__.__name__,
                                                                                    "\n\t".join(error_msgs)))
        return model


class BertEmbeddings(nn.Module):
    """Reference basebert.py:284-321: all three tables are built with padding_idx = 0. The parameters of the text half of the
    joint embedding; BertModel.forward launches it together with the image half."""

    def __init__(self, config):
        super(BertEmbeddings, self).__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=0)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size, padding_idx=0)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size, padding_idx=0)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_ids, token_type_ids=None):
        raise NotImplementedError("vilbert.basebert: the text and image embeddings run as one joint kernel - call BertModel")


class BertImageEmbeddings(nn.Module):
    """Reference basebert.py:324-359: 2048 -> H feature projection + token-type row + 5 -> H location projection + LayerNorm.
    The parameters of the image half of the joint embedding."""

    def __init__(self, config):
        super(BertImageEmbeddings, self).__init__()
        self.image_embeddings = nn.Linear(IMAGE_FEATURE_SIZE, config.hidden_size)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size, padding_idx=0)
        self.image_location_embeddings = nn.Linear(5, config.hidden_size)
        self.LayerNorm = BertLayerNorm(config.hidden_size, eps=1e-12)
        self.dropout = nn.Dropout(config.hidden_dropout_prob)

    def forward(self, input_ids, input_loc, token_type_ids=None):
        raise NotImplementedError("vilbert.basebert: the text and image embeddings run as one joint kernel - call BertModel")


class BertEncoder(nn.Module):
    """Reference basebert.py:488-504: a stack of plain BERT layers over the joint sequence."""

    def __init__(self, config):
        super(BertEncoder, self).__init__()
        layer_config = _layer_config(config)
        self.layer = nn.ModuleList([BertLayer(layer_config) for _ in range(config.num_hidden_layers)])

    def forward(self, hidden_states, attention_mask, output_all_encoded_layers=True):
        all_encoder_layers = []
        for layer_module in self.layer:
            hidden_states, _ = layer_module(hidden_states, attention_mask)
            if output_all_encoded_layers:
                all_encoder_layers.append(hidden_states)
        if not output_all_encoded_layers:
            all_encoder_layers.append(hidden_states)
        return all_encoder_layers


class BertPooler(nn.Module):
    """tanh(dense(h[:, 0])), reference basebert.py:507-519: the first-token rows are read in place through the GEMM's row stride,
    the tanh is its own small kernel (the GEMM epilogues implement none / GELU / ReLU / swish)."""

    def __init__(self, config):
        super(BertPooler, self).__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.activation = nn.Tanh()

    def forward(self, hidden_states):
        return F.tanh(F.linear(hidden_states[:, 0], self.dense.weight, self.dense.bias))


class BertImagePredictionHead(nn.Module):
    """Reference basebert.py:622-634: the TEXT head transform and a 1601-wide decoder."""

    def __init__(self, config, bert_model_embedding_weights):
        super(BertImagePredictionHead, self).__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(bert_model_embedding_weights.size(1), IMAGE_TARGET_SIZE)

    def forward(self, hidden_states):
        return F.linear(self.transform(hidden_states), self.decoder.weight, self.decoder.bias)


class BertPreTrainingHeads(nn.Module):
    """Reference basebert.py:637-656."""

    def __init__(self, config, bert_model_embedding_weights):
        super(BertPreTrainingHeads, self).__init__()
        self.predictions = BertLMPredictionHead(config, bert_model_embedding_weights)
        self.seq_relationship = nn.Linear(config.hidden_size, 2)
        self.imagePredictions = BertImagePredictionHead(config, bert_model_embedding_weights)

    def forward(self, sequence_output_t, sequence_output_v, pooled_output):
        img_prediction_scores = self.imagePredictions(sequence_output_v)
        prediction_scores = self.predictions(sequence_output_t)
        seq_relationship_score = F.linear(pooled_output, self.seq_relationship.weight, self.seq_relationship.bias)
        return img_prediction_scores, prediction_scores, seq_relationship_score


class BertModel(BertPreTrainedModel):
    """Reference basebert.py:659-774."""

    def __init__(self, config):
        super(BertModel, self).__init__(config)
        _check_head_dim(config.hidden_size // config.num_attention_heads, "basebert.BertModel")
        _act_name(config.hidden_act)
        self.image_embeddings = BertImageEmbeddings(config)
        self.embeddings = BertEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.pooler = BertPooler(config)
        self.apply(self.init_bert_weights)

    def embed(self, input_txt, input_imgs, image_loc, token_type_ids=None, attention_mask=None, image_attention_mask=None):
        """-> (joint embedding [B, T + R, H] after its dropout, additive attention mask [B, T + R])."""
        txt, img = self.embeddings, self.image_embeddings
        if token_type_ids is None:
            token_type_ids = torch.zeros_like(input_txt)
        if txt.dropout.p != img.dropout.p:
            raise NotImplementedError("basebert: the two embedding dropouts share one mask draw and need the same p")
        proj = F.linear(input_imgs.float(), img.image_embeddings.weight, img.image_embeddings.bias)
        # (the image token-type ids are all ones, :726-728: row 1 of the table is added to every region)
        out, add_mask = F.joint_embed_ln(
            input_txt.long(), token_type_ids.long(), txt.word_embeddings.weight, txt.position_embeddings.weight,
            txt.token_type_embeddings.weight, txt.LayerNorm.weight, txt.LayerNorm.bias, proj, image_loc.float(),
            img.image_location_embeddings.weight, img.image_location_embeddings.bias, img.token_type_embeddings.weight,
            img.LayerNorm.weight, img.LayerNorm.bias, txt.LayerNorm.variance_epsilon, attention_mask, image_attention_mask)
        return _dropout(out, txt.dropout), add_mask

    def forward(self, input_txt, input_imgs, image_loc, token_type_ids=None, attention_mask=None,
                image_attention_mask=None, output_all_encoded_layers=True):
        _require_fp32_stream("basebert.BertModel")
        embedding_output, add_mask = self.embed(input_txt, input_imgs, image_loc, token_type_ids, attention_mask,
                                                image_attention_mask)
        encoded_layers = self.encoder(embedding_output, add_mask.unsqueeze(1).unsqueeze(2),
                                      output_all_encoded_layers=output_all_encoded_layers)
        pooled_output = self.pooler(encoded_layers[-1])
        if not output_all_encoded_layers:
            encoded_layers = encoded_layers[-1]
        return encoded_layers, pooled_output


class BertForMultiModalPreTraining(BertPreTrainedModel):
    """Reference basebert.py:777-890, construction only: the reference's own forward cannot run - it calls ``self.cls`` with
    four arguments where BertPreTrainingHeads.forward takes three (:864-866) and returns the undefined name
    ``prediction_scores`` (:890) - so there is no behaviour to reproduce."""

    def __init__(self, config):
        super(BertForMultiModalPreTraining, self).__init__(config)
        self.bert = BertModel(config)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        self.apply(self.init_bert_weights)
        self.vis_criterion = nn.KLDivLoss(reduction="none")
        self.loss_fct = CrossEntropyLoss(ignore_index=-1)

    def forward(self, input_ids, image_feat, image_target, image_loc, token_type_ids=None, attention_mask=None,
                image_attention_mask=None, masked_lm_labels=None, image_label=None, next_sentence_label=None):
        raise NotImplementedError(
            "basebert.BertForMultiModalPreTraining.forward: the reference's forward cannot run (basebert.py:864-866 calls "
            "self.cls with four arguments, :890 returns an undefined name); pre-train with vilbert.vilbert")


class SimpleClassifier(nn.Module):
    """weight_norm(Linear) -> ReLU -> Dropout -> weight_norm(Linear), reference basebert.py:965-978 (``main.0`` / ``main.3``
    with ``weight_g`` / ``weight_v``, dim=None: one norm over the whole matrix). The effective weights g * v / |v| are formed
    by torch (two small parameter-sized ops, differentiable); bias, ReLU and the dropout are the first GEMM's epilogue."""

    def __init__(self, in_dim, hid_dim, out_dim, dropout):
        super(SimpleClassifier, self).__init__()
        layers = [weight_norm(nn.Linear(in_dim, hid_dim), dim=None), nn.ReLU(), nn.Dropout(dropout, inplace=True),
                  weight_norm(nn.Linear(hid_dim, out_dim), dim=None)]
        self.main = nn.Sequential(*layers)

    @staticmethod
    def _weight(linear):
        return linear.weight_v * (linear.weight_g / torch.norm(linear.weight_v))

    def forward(self, x):
        fc0, _, drop, fc3 = self.main
        hidden = F.linear(x, self._weight(fc0), fc0.bias, act="relu", drop_p=_drop_p(drop))
        return F.linear(hidden, self._weight(fc3), fc3.bias)


class BaseBertForVLTasks(BertPreTrainedModel):
    """Reference basebert.py:893-962: by default every head is computed on every forward, as there. `set_active_heads` names
    the heads a step needs; the others are None in the returned tuple and launch nothing."""

    def __init__(self, config, num_labels, dropout_prob=0.1, default_gpu=True):
        super(BaseBertForVLTasks, self).__init__(config)
        self.num_labels = num_labels
        self.bert = BertModel(config)
        self.dropout = nn.Dropout(dropout_prob)
        self.cls = BertPreTrainingHeads(config, self.bert.embeddings.word_embeddings.weight)
        self.vil_prediction = SimpleClassifier(config.hidden_size, config.hidden_size * 2, num_labels, 0.5)
        self.vil_logit = nn.Linear(config.hidden_size, 1)
        self.vision_logit = nn.Linear(config.hidden_size, 1)
        self.linguisic_logit = nn.Linear(config.hidden_size, 1)
        self.active_heads = None        # None: all seven (set_active_heads)
        self.apply(self.init_bert_weights)

    def set_active_heads(self, names=None):
        """Which of the seven outputs (BASEBERT_HEADS) the following forwards compute: a name or an iterable of names; None (the
        default) = all of them, the reference's behaviour. An unselected head is None in the returned tuple and launches
        nothing: by default every step runs the vocabulary-wide decoder over all text rows and the 1,601-wide one over all
        image rows. A dropout site of an unselected head still draws its seed, so the masks of the selected heads are those
        of the all-heads forward."""
        if names is None:
            self.active_heads = None
            return
        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in BASEBERT_HEADS]
        if unknown:
            raise ValueError("set_active_heads: unknown head name(s) %s - valid names: %s"
                             % (", ".join(repr(n) for n in unknown), ", ".join(BASEBERT_HEADS)))
        self.active_heads = tuple(n for n in BASEBERT_HEADS if n in names)

    def forward(self, input_txt, input_imgs, image_loc, token_type_ids=None, attention_mask=None,
                image_attention_mask=None, co_attention_mask=None, output_all_encoded_layers=False):
        heads = getattr(self, "active_heads", None)
        want = frozenset(BASEBERT_HEADS if heads is None else heads)
        sequence_output, pooled_output = self.bert(input_txt, input_imgs, image_loc, token_type_ids, attention_mask,
                                                   image_attention_mask, output_all_encoded_layers=output_all_encoded_layers)
        if output_all_encoded_layers:          # (the reference slices the list here and fails; the last layer is what it means)
            sequence_output = sequence_output[-1]
        n_tok = input_txt.size(1)
        # the two segments of the joint output, each split off once and only where a head reads it
        sequence_output_t = sequence_output_v = None
        if want & {"linguisic_prediction", "linguisic_logit"}:
            sequence_output_t = sequence_output[:, :n_tok].contiguous()
        if want & {"vision_prediction", "vision_logit"}:
            sequence_output_v = sequence_output[:, n_tok:].contiguous()

        cls = self.cls
        vision_prediction = linguisic_prediction = vil_binary_prediction = None
        if "vision_prediction" in want:
            vision_prediction = cls.imagePredictions(sequence_output_v)
        if "linguisic_prediction" in want:
            linguisic_prediction = cls.predictions(sequence_output_t)
        if "vil_binary_prediction" in want:
            vil_binary_prediction = F.linear(pooled_output, cls.seq_relationship.weight, cls.seq_relationship.bias)

        vil_prediction = vil_logit = vision_logit = linguisic_logit = None
        if "vil_prediction" in want:
            vil_prediction = self.vil_prediction(pooled_output)
        else:
            _skip_dropout_seed(self.vil_prediction.main[2])
        if "vil_logit" in want:
            vil_logit = F.linear(pooled_output, self.vil_logit.weight, self.vil_logit.bias)
        if "vision_logit" not in want:
            _skip_dropout_seed(self.dropout)
        else:
            # like the reference this needs image_attention_mask (:949-951 fail on None)
            region_mask = ops.additive_mask(image_attention_mask).unsqueeze(2)
            vision_logit = F.linear(_dropout(sequence_output_v, self.dropout), self.vision_logit.weight,
                                    self.vision_logit.bias, residual=region_mask)
        if "linguisic_logit" not in want:
            _skip_dropout_seed(self.dropout)
        else:
            linguisic_logit = F.linear(_dropout(sequence_output_t, self.dropout), self.linguisic_logit.weight,
                                       self.linguisic_logit.bias)
        return (vil_prediction, vil_logit, vil_binary_prediction, vision_prediction, vision_logit, linguisic_prediction,
                linguisic_logit)
