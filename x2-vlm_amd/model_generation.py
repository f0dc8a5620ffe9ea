"""Captioning fine-tune on the MI355X stages (models/model_generation.py:54-111, Captioning_MLM.py).

  XVLMForMLMCaptioning   training forward: the label-smoothed, weight-normalised MLM loss of the UniLM-style captioning collate

The text encoder runs every layer with the collate's [B, L, L] attention mask (tril, or FG-free: [MASK] columns zeroed but for their
own diagonal entry) through the 2-D masked attention kernels, embeds explicit (repeating) position ids, and forms the loss inside the
decoder GEMM (kernels.mlm_ls_fwd / _bwd): the [B * max_masks, vocab] logits are never written.
"""
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from .xvlm import XVLMBase


class _SmoothedTarget(nn.Module):
    """The state LabelSmoothingLoss keeps (model_generation.py:31-34): the off-label target row `one_hot` [1, V] (ls / (V - 2), 0 at the
    ignored id), a buffer of the reference's state dict (`crit_mask_lm_smoothed.one_hot`).  The loss itself runs in the fused MLM head."""

    def __init__(self, label_smoothing, vocab_size, ignore_index):
        super().__init__()
        one_hot = torch.full((vocab_size,), label_smoothing / (vocab_size - 2))
        one_hot[ignore_index] = 0
        self.register_buffer("one_hot", one_hot.unsqueeze(0))


def _build_tokenizer(config, text_config):
    """The reference builds the text encoder's tokenizer from its directory (BERT encoders: a BertTokenizer on its vocab.txt - the only
    text encoders this path builds); the training forward needs only its [CLS] id and vocabulary size.  Where that tokenizer cannot be
    built (no transformers, or no vocab.txt) config["cls_token_id"] must say the ignored id - a wrong one would silently change the loss -
    and the vocabulary is the text encoder's.  Where both exist they must agree."""
    path = config.get("text_encoder", "")
    try:
        from transformers import BertTokenizer
    except ImportError:
        BertTokenizer = None
    if BertTokenizer is not None and path and os.path.exists(os.path.join(path, "vocab.txt")):
        tok = BertTokenizer.from_pretrained(path)
        if "cls_token_id" in config and int(config["cls_token_id"]) != tok.cls_token_id:
            raise ValueError("config cls_token_id %d != the tokenizer's %d" % (config["cls_token_id"], tok.cls_token_id))
        return tok
    if "cls_token_id" not in config:
        raise ValueError("no tokenizer could be built from %r (transformers and a vocab.txt are needed): set config['cls_token_id'], the "
                         "id the captioning loss ignores" % path)
    return SimpleNamespace(cls_token_id=int(config["cls_token_id"]), vocab_size=int(text_config.vocab_size), cls_token="[CLS]")


class XVLMForMLMCaptioning(XVLMBase):
    def __init__(self, config):
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=False, use_matching_loss=False,
                         use_mlm_loss=True, use_bbox_loss=False, config_text=None)
        self.tokenizer = _build_tokenizer(config, self.text_encoder.config)
        if hasattr(self.tokenizer, "tokenize"):
            self.prompt_ids = self.tokenizer.convert_tokens_to_ids([self.tokenizer.cls_token] + self.tokenizer.tokenize(config.get("prompt", "")))
        else:
            self.prompt_ids = [self.tokenizer.cls_token_id]
        self.label_smoothing = float(config["label_smoothing"])
        assert 0.0 < self.label_smoothing <= 1.0          # LabelSmoothingLoss's own check
        self.ignore_index = int(self.tokenizer.cls_token_id)
        self.tgt_vocab_size = int(self.tokenizer.vocab_size)
        assert self.tgt_vocab_size == self.text_encoder.config.vocab_size, \
            "tokenizer vocabulary %d != text encoder vocabulary %d" % (self.tgt_vocab_size, self.text_encoder.config.vocab_size)
        self.crit_mask_lm_smoothed = _SmoothedTarget(self.label_smoothing, self.tgt_vocab_size, self.ignore_index)

    def load_pretrained(self, ckpt_rpath, config, is_eval=False):
        from . import checkpoint
        if is_eval:
            state_dict = checkpoint.load_pretrained(self, ckpt_rpath, config, is_eval=True)
        else:
            state_dict = checkpoint.load_pretrained(self, ckpt_rpath, config, load_text=False)
        msg = self.load_state_dict(state_dict, strict=False)
        print("load checkpoint from %s" % ckpt_rpath)
        print("missing_keys: ", [p for p in msg.missing_keys])
        print("unexpected_keys: ", msg.unexpected_keys)

    def forward(self, image, input_ids_masked, attention_mask, position_ids, masked_pos, masked_ids, masked_weight):
        loss, _ = self.forward_with_scores(image, input_ids_masked, attention_mask, position_ids, masked_pos, masked_ids, masked_weight)
        return loss

    def forward_with_scores(self, image, input_ids_masked, attention_mask, position_ids, masked_pos, masked_ids, masked_weight,
                            keep_scores=False):
        """(loss, prediction_scores [B, n_mask, V] fp32 when keep_scores else None)."""
        image_embeds, image_atts = self.get_vision_embeds(image)
        te = self.text_encoder
        h = te.bert(input_ids_masked, attention_mask=attention_mask, position_ids=position_ids, encoder_hidden_states=image_embeds,
                    encoder_attention_mask=image_atts).last_hidden_state
        loss, _, logits = te.smoothed_mlm_loss_from_hidden(h, masked_pos, masked_ids.reshape(-1).to(torch.int64).contiguous(), masked_weight,
                                                           self.ignore_index, self.label_smoothing, keep_logits=keep_scores)
        scores = None
        if keep_scores:
            scores = logits[:, :self.tgt_vocab_size].reshape(masked_pos.shape[0], masked_pos.shape[1], -1)
        return loss, scores

    def generate(self, *args, **kwargs):
        raise NotImplementedError("XVLMForMLMCaptioning.generate (beam search over cached layer states) is the follow-up to the "
                                  "captioning training step and is not implemented on the HIP path yet")
