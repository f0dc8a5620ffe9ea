"""Captioning fine-tune and inference on the MI355X stages (models/model_generation.py:54-397, Captioning_MLM.py).

  XVLMForMLMCaptioning   training forward: the label-smoothed, weight-normalised MLM loss of the UniLM-style captioning collate
                         generate / beam_search: beam search over cached K/V (decode.py), HIP device only

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
        tok.add_special_tokens({"bos_token": tok.cls_token})          # the reference's build_tokenizer: "always use cls and sep"
        tok.add_special_tokens({"eos_token": tok.sep_token})
        if "cls_token_id" in config and int(config["cls_token_id"]) != tok.cls_token_id:
            raise ValueError("config cls_token_id %d != the tokenizer's %d" % (config["cls_token_id"], tok.cls_token_id))
        return tok
    if "cls_token_id" not in config:
        raise ValueError("no tokenizer could be built from %r (transformers and a vocab.txt are needed): set config['cls_token_id'], the "
                         "id the captioning loss ignores" % path)
    # generate() also needs the ids of [SEP] (the EOS) and [MASK]: config["eos_token_id"] / config["mask_token_id"], checked when it is called
    opt = {k: int(config[k]) if k in config else None for k in ("eos_token_id", "mask_token_id")}
    return SimpleNamespace(cls_token_id=int(config["cls_token_id"]), vocab_size=int(text_config.vocab_size), cls_token="[CLS]", **opt)


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

    _HOST_PATH = "%s runs on the HIP path; a host (CPU) path is a possible follow-up and is not implemented"

    def generate(self, image, num_beams=3, min_length=5, max_length=20, length_penalty=0, forbid_duplicate_ngrams=True, ngram_size=3):
        """Captions of `image` [B, 3, R, R] (a HIP tensor) by beam search: decoded strings with a real tokenizer, the id lists with the
        fallback tokenizer namespace (which needs config["eos_token_id"] and config["mask_token_id"]).

        Sizes as the reference (model_generation.py:113-127): length = input_ids.size(0) + max_length - the BATCH size, not the prompt
        length - so the search runs bsz + max_length - len(prompt_ids) steps.  Kept as it is (the goldens come from the real reference);
        like the reference there is no early exit when every beam has ended."""
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise NotImplementedError(self._HOST_PATH % "generate")
        from . import decode
        dev, batch = image.device, image.shape[0]
        prompt = torch.tensor([self.prompt_ids] * batch, dtype=torch.long, device=dev)
        length, _ = decode.generation_lengths(batch, prompt.shape[1], max_length, self.text_encoder.config.max_position_embeddings)
        causal = torch.ones(length, length, dtype=torch.long, device=dev).tril_()
        output_ids = self.beam_search(image, prompt, torch.zeros(batch, length, dtype=torch.long, device=dev),
                                      torch.arange(length, device=dev).repeat(batch, 1), causal.repeat(batch, 1, 1), num_beams=num_beams,
                                      min_length=min_length, length_penalty=length_penalty, forbid_duplicate_ngrams=forbid_duplicate_ngrams,
                                      ngram_size=ngram_size)
        if hasattr(self.tokenizer, "decode"):
            return [self.tokenizer.decode(ids, skip_special_tokens=True) for ids in output_ids]
        return output_ids

    def generation_token_ids(self):
        """(eos id, [MASK] id) of the tokenizer; the fallback namespace has them only from config["eos_token_id"] / config["mask_token_id"]."""
        for k in ("eos_token_id", "mask_token_id"):
            if getattr(self.tokenizer, k, None) is None:
                raise ValueError("no tokenizer could be built (transformers and a vocab.txt are needed): set config['%s'], which generate needs" % k)
        return int(self.tokenizer.eos_token_id), int(self.tokenizer.mask_token_id)

    def beam_search(self, image, input_ids, token_type_ids, position_ids, attention_mask, num_beams=3, min_length=5, length_penalty=0,
                    forbid_duplicate_ngrams=True, ngram_size=3, _forced=None, _return_traces=False, _use_cache=True):
        """The reference's beam search (model_generation.py:139-397) over per-row K/V caches (decode.py) -> the padded pred_seq id lists
        [B][length].  token_type_ids [B, length] gives the output length, position_ids [B, length], attention_mask [B, length, length]
        (tril).  Inference only: runs in eval mode under no_grad, the training flag is restored.

        Test seam (not part of the mirrored API): _forced=(step_ids, back_ptrs), per step [B, K], are followed instead of the search's own
        selections - the total scores and the ids such a run returns mean nothing (a forced id outside its parent's K candidates scores NaN); _return_traces adds a dict with, per step, the [S, K] values and ids of x2_logprob_topk, the [S, V] log-scores when
        V <= 1024 and the [MASK]-row logits, plus the [T, B, K] total_scores / step_ids / back_ptrs; _use_cache=False recomputes the whole
        prefix every step through the full-sequence forward (the measured baseline)."""
        if not isinstance(image, torch.Tensor) or not image.is_cuda:
            raise NotImplementedError(self._HOST_PATH % "beam_search")
        self.generation_token_ids()
        from . import decode
        was_training = self.training
        self.eval()
        try:
            return decode.beam_search(self, image, input_ids, token_type_ids, position_ids, attention_mask, num_beams=num_beams,
                                      min_length=min_length, length_penalty=length_penalty, forbid_duplicate_ngrams=forbid_duplicate_ngrams,
                                      ngram_size=ngram_size, _forced=_forced, _return_traces=_return_traces, _use_cache=_use_cache)
        finally:
            self.train(was_training)
