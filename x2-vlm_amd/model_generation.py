"""Captioning fine-tune and inference, VQA fine-tune and answer ranking on the MI355X stages (models/model_generation.py:54-619,
Captioning_MLM.py, VQA.py).

  XVLMForMLMCaptioning   training forward: the label-smoothed, weight-normalised MLM loss of the UniLM-style captioning collate
                         generate / beam_search: beam search over cached K/V (decode.py), HIP device only
  XVLMForVQA             forward(train=True): the weighted per-answer LM loss of the answer decoder, the question states shared by a
                         question's answer rows, HIP device only
                         forward(train=False) / rank_answer: the k candidate answers with the likeliest first token, re-ranked by the
                         answer decoder's sequence log-probability, HIP device only

The text encoder runs every layer with the collate's [B, L, L] attention mask (tril, or FG-free: [MASK] columns zeroed but for their
own diagonal entry) through the 2-D masked attention kernels, embeds explicit (repeating) position ids, and forms the loss inside the
decoder GEMM (kernels.mlm_ls_fwd / _bwd): the [B * max_masks, vocab] logits are never written.
"""
import contextlib
import copy
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import kernels as K
from . import ops
from .xbert import BertLMHeadModel
from .xvlm import XVLMBase


@contextlib.contextmanager
def _inference(model):
    """eval mode under no_grad; the training flag is restored"""
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        model.train(was_training)


def _load_pretrained(model, ckpt_rpath, config, is_eval, remap=None, hide=None):
    """load_pretrained of both models: the checkpoint through checkpoint.load_pretrained (a pre-training one, is_eval False, without its
    text parameters' renaming and then through `remap`), loaded non-strictly; missing keys containing `hide` are not printed."""
    from . import checkpoint
    if is_eval:
        state_dict = checkpoint.load_pretrained(model, ckpt_rpath, config, is_eval=True)
    else:
        state_dict = checkpoint.load_pretrained(model, ckpt_rpath, config, load_text=False)
        if remap is not None:
            remap(state_dict)
    msg = model.load_state_dict(state_dict, strict=False)
    print("load checkpoint from %s" % ckpt_rpath)
    print("missing_keys: ", [p for p in msg.missing_keys if hide is None or hide not in p])
    print("unexpected_keys: ", msg.unexpected_keys)
    return msg


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
        _load_pretrained(self, ckpt_rpath, config, is_eval)

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

    def generate(self, image, num_beams=3, min_length=5, max_length=20, length_penalty=0, forbid_duplicate_ngrams=True, ngram_size=3):
        """Captions of `image` [B, 3, R, R] (a HIP tensor) by beam search: decoded strings with a real tokenizer, the id lists with the
        fallback tokenizer namespace (which needs config["eos_token_id"] and config["mask_token_id"]).

        Sizes as the reference (model_generation.py:113-127): length = input_ids.size(0) + max_length - the BATCH size, not the prompt
        length - so the search runs bsz + max_length - len(prompt_ids) steps.  Kept as it is (the goldens come from the real reference);
        like the reference there is no early exit when every beam has ended."""
        ops.require_hip(image, "generate")
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
        ops.require_hip(image, "beam_search")
        self.generation_token_ids()
        from . import decode
        with _inference(self):
            return decode.beam_search(self, image, input_ids, token_type_ids, position_ids, attention_mask, num_beams=num_beams,
                                      min_length=min_length, length_penalty=length_penalty, forbid_duplicate_ngrams=forbid_duplicate_ngrams,
                                      ngram_size=ngram_size, _forced=_forced, _return_traces=_return_traces, _use_cache=_use_cache)


class XVLMForVQA(XVLMBase):
    """The reference's generative VQA model, ranking a closed answer list at inference (model_generation.py:409-619): `text_encoder` is the
    bare 12 + n layer BertModel reading the image, `text_decoder` a BertLMHeadModel of num_dec_layers layers, every one with cross-attention
    to the question states.

    rank_answer on the HIP path, no host synchronisation between its stages:
      1. the decoder on the [B, 1] start ids and the full head on those B rows -> first-step logits [B, Vp] (kept: B x V is small)
      2. kernels.answer_topk: log-softmax, gathered at the Na answers' first tokens, the k best per question (LOG-probabilities: the
         reference's softmax(...).log() underflows below 1e-38)
      3. kernels.vqa_candidates: ids, next-token labels, the row -> question map and the additive tril x padding mask of the S = B * k rows
      4. ONE decoder pass over the S rows; the B question states are shared through kv_idx (cross-attention K/V projected once per
         question, not per candidate - the reference's tile() without the copy)
      5. the head's transform and kernels.mlm_ce_rows on positions 0 .. La - 2 of every row: loss per scored token, logits never stored
      6. kernels.vqa_rerank: score = first-token log-probability - summed losses, softmax over k, sorted.
    Ties (candidates sharing a first token tie exactly in stage 2): the lower candidate index / slot comes first, where torch.topk leaves
    the order open.

    The training step (forward(train=True), model_generation.py:517-550), no host synchronisation either:
      1. kernels.vqa_train_rows: from the prefix sum of k the row -> question map, the next-token labels, the additive tril x padding mask
         and c = weights / B of the S answer rows, in one launch
      2. ONE decoder pass over the S rows, the B question states shared through kv_idx (the reference stacks k[b] copies of each); their
         gradient comes back summed over a question's rows
      3. engine.SeqLmLossFn: the per-answer summed cross-entropy and sum_s c[s] * loss[s] from softmax statistics reduced inside the decoder
         GEMM; the backward recomputes the GEMM and writes the logit gradient as bf16.
    Extension over the reference: with k a DEVICE tensor, rows s >= sum(k) are padding (a captured graph has a fixed S while sum(k) changes
    from batch to batch): they need valid token ids, get weight 0, no labels and the last question's states, and add exactly zero to the loss
    and to every gradient."""

    def __init__(self, config):
        if config["text_encoder"] == "data/roberta-base":
            raise NotImplementedError("RoBERTa text encoders / decoders are outside the X2VLM-base/large hot path")
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=False, use_matching_loss=False,
                         use_mlm_loss=False, use_bbox_loss=False, config_text=None)
        assert isinstance(config["pad_token_id"], int)
        self.pad_token_id = config["pad_token_id"]
        config_enc = self.text_encoder.config
        self.num_text_layers = config_enc.fusion_layer
        self.num_cross_layers = config_enc.num_hidden_layers - config_enc.fusion_layer
        assert config["num_dec_layers"] in [self.num_cross_layers, self.num_cross_layers // 2], "initialization not implemented"
        self.num_dec_layers = config["num_dec_layers"]
        config_dec = copy.deepcopy(config_enc)
        config_dec.encoder_width = config_enc.hidden_size
        config_dec.fusion_layer = 0
        config_dec.num_hidden_layers = config["num_dec_layers"]
        self.cross_encoder_width = config_enc.encoder_width          # the vision width
        self.dec_encoder_width = config_enc.hidden_size
        self.text_decoder = BertLMHeadModel(config=config_dec)
        if config.get("large_lr_for_dec", False):
            self.init_params = ["text_decoder." + n for n, _ in self.text_decoder.named_parameters()]
        elif self.dec_encoder_width != self.cross_encoder_width:
            self.init_params = ["text_decoder." + n for n, _ in self.text_decoder.named_parameters()
                                if ("crossattention.self.key" in n) or ("crossattention.self.value" in n)]
        else:
            self.init_params = []

    def map_pretrained_state(self, state_dict, text_encoder_name=""):
        """A pre-training checkpoint's keys for this model, in place (model_generation.py:461-507): every key with a `bert.` infix also
        appears without it (the bare text encoder's names); text_encoder.bert.* moves to text_decoder.bert.* - embeddings and head as
        they are, layers >= num_text_layers renumbered from 0 (only the odd-numbered ones, in pairs, when the decoder has half the cross
        layers), layers below dropped, cross-attention key / value dropped when the question width differs from the vision width."""
        infix = "roberta." if "roberta" in text_encoder_name else "bert."
        halved = self.num_dec_layers == self.num_cross_layers // 2
        for key in list(state_dict.keys()):
            if infix in key:
                state_dict[key.replace(infix, "")] = state_dict[key]
            if "text_encoder." not in key:
                continue
            target = key
            if "layer." in key:
                parts = key.split(".")
                layer = int(parts[4])                                       # text_encoder.bert.encoder.layer.<n>
                cross_kv = ("crossattention.self.key" in key) or ("crossattention.self.value" in key)
                if layer < self.num_text_layers or (halved and layer % 2 == 0) or \
                        (self.dec_encoder_width != self.cross_encoder_width and cross_kv):
                    del state_dict[key]
                    continue
                if halved:
                    parts[4] = str((layer - self.num_text_layers) // 2)
                elif self.num_dec_layers == self.num_cross_layers:
                    parts[4] = str(layer - self.num_text_layers)
                else:
                    raise ValueError
                target = ".".join(parts)
            state_dict[target.replace("text_encoder", "text_decoder")] = state_dict.pop(key)
        return state_dict

    def load_pretrained(self, ckpt_rpath, config, is_eval=False):
        def remap(state_dict):
            print("### Loading pretrained text encoder", flush=True)
            self.map_pretrained_state(state_dict, config["text_encoder"])
        return _load_pretrained(self, ckpt_rpath, config, is_eval, remap, hide="vision_encoder")

    def forward(self, image, quesiton, answer=None, k=None, weights=None, train=True, _fused=True, _stage1_ids=None, _return_traces=False):
        """train=True: the loss of the reference's training step, a differentiable fp32 device scalar:
            sum_s weights[s] * (sum over t of CE(logits[s, t], answer_ids[s, t + 1])) / image.size(0)
        `answer` (.input_ids / .attention_mask [S, La], 2 <= La <= 128) holds one row per (question, answer) pair, the k[b] rows of question b
        next to each other; a next token equal to pad_token_id is not scored; weights is fp32 [S] and gets no gradient.  k is a list or host
        tensor (checked: one entry >= 1 per image, sum(k) == S) or a device int tensor [B] that is never read back: the caller guarantees
        k[b] >= 1 and sum(k) <= S, and rows s >= sum(k) are padding (see the class docstring).  self.training decides the dropout.

        train=False: (topk_ids int64 [B, k] indices into the answer list, topk_probs fp32 [B, k]) for `image` [B, 3, R, R], the tokenised
        questions (`quesiton`, the reference's spelling: .input_ids / .attention_mask [B, Lq]) and the tokenised answer LIST `answer`
        ([Na, La], every row starting with the same start token).  Runs in eval mode under no_grad; the training flag is restored.  The
        underscored keywords are rank_answer's test seam."""
        if train:
            return self._train_step(image, quesiton, answer, k, weights)
        ops.require_hip(image, "XVLMForVQA.forward")
        with _inference(self):
            image_embeds, image_atts = self.get_vision_embeds(image)
            question_states = self.text_encoder(quesiton.input_ids, attention_mask=quesiton.attention_mask, encoder_hidden_states=image_embeds,
                                                encoder_attention_mask=image_atts, return_dict=True).last_hidden_state
            return self.rank_answer(question_states, quesiton.attention_mask, answer.input_ids, answer.attention_mask, k, _fused=_fused,
                                    _stage1_ids=_stage1_ids, _return_traces=_return_traces)

    def _train_step(self, image, quesiton, answer, k, weights):
        ops.require_hip(image, "XVLMForVQA.forward(train=True): the VQA training step")
        B = image.size(0)

        def refuse(what):
            return NotImplementedError("XVLMForVQA.forward(train=True): the VQA training step takes one k per image and one weight per answer "
                                       "row, answers of 2 to 128 tokens; got " + what)
        if answer is None or k is None or weights is None:
            raise refuse("answer, k or weights missing")
        dev = image.device
        answer_ids = answer.input_ids.to(dev).to(torch.int64).contiguous()
        answer_atts = answer.attention_mask.to(dev).to(torch.int64).contiguous()
        if answer_ids.dim() != 2 or answer_atts.shape != answer_ids.shape or not 2 <= answer_ids.shape[1] <= 128:
            raise refuse("answer ids %s, attention mask %s" % (tuple(answer_ids.shape), tuple(answer_atts.shape)))
        S = answer_ids.shape[0]
        weights = torch.as_tensor(weights, dtype=torch.float32).detach().to(dev).reshape(-1).contiguous()
        if weights.numel() != S:
            raise refuse("%d weights for %d answer rows" % (weights.numel(), S))
        if isinstance(k, torch.Tensor) and k.is_cuda:
            if k.numel() != B or k.dtype not in (torch.int32, torch.int64):
                raise refuse("k of %d %s entries for %d images" % (k.numel(), k.dtype, B))
            offs = torch.zeros(B + 1, device=dev, dtype=torch.int32)
            offs[1:] = torch.cumsum(k.reshape(-1), 0)
        else:
            ks = [int(n) for n in (k.tolist() if isinstance(k, torch.Tensor) else k)]
            if len(ks) != B or min(ks) < 1 or sum(ks) != S:
                raise refuse("k = %s for %d images and %d answer rows" % (ks, B, S))
            offs = torch.tensor([sum(ks[:b]) for b in range(B + 1)], dtype=torch.int32).to(dev)
        image_embeds, image_atts = self.get_vision_embeds(image)
        question_states = self.text_encoder(quesiton.input_ids, attention_mask=quesiton.attention_mask, encoder_hidden_states=image_embeds,
                                            encoder_attention_mask=image_atts, return_dict=True).last_hidden_state
        kv_idx, labels, mask2d, c = K.vqa_train_rows(offs, answer_ids, answer_atts, weights, self.pad_token_id)
        row_atts = quesiton.attention_mask.index_select(0, kv_idx.long())
        out = self.text_decoder(answer_ids, encoder_hidden_states=question_states.contiguous(), encoder_attention_mask=row_atts, kv_idx=kv_idx,
                                self_mask2d=mask2d, reduction="none", _next_labels=labels, _seq_weights=c)
        return out.total

    def rank_answer(self, question_states, question_atts, answer_ids, answer_atts, k, _fused=True, _stage1_ids=None, _return_traces=False):
        """question_states [B, Lq, Hd] fp32, question_atts [B, Lq], answer_ids / answer_atts int64 [Na, La] -> (topk_ids int64 [B, k],
        topk_probs fp32 [B, k]), best first.  1 <= k <= min(Na, 256), Na <= 65536, 2 <= La <= 128.

        Test seam (not part of the mirrored API): _fused=False runs the same stages with the [S * (La - 1), V] logits materialised and the
        candidate bookkeeping in torch (the measured baseline of probes/bench_vqa_rank.py); _stage1_ids int [B, k] replaces the first stage's
        selection (their log-probabilities are looked up); _return_traces adds a dict: logits0 [B, V], logp_first [B, Na], stage1_logp /
        stage1_ids [B, k], loss_rows [S, La - 1], scores [B, k] in stage-1 slot order."""
        ops.require_hip(question_states, "XVLMForVQA.rank_answer")
        with _inference(self):
            return self._rank_answer(question_states, question_atts, answer_ids, answer_atts, int(k), _fused, _stage1_ids, _return_traces)

    def _rank_answer(self, question_states, question_atts, answer_ids, answer_atts, k, fused, stage1_ids, want_traces):
        dec = self.text_decoder
        V = dec.config.vocab_size
        dev = question_states.device
        B, Hd = question_states.shape[0], question_states.shape[2]
        Na, La = answer_ids.shape
        if not (1 <= k <= min(Na, 256) and Na <= 65536 and 2 <= La <= 128):
            raise ValueError("rank_answer: k=%d Na=%d La=%d outside 1 <= k <= min(Na, 256), Na <= 65536, 2 <= La <= 128" % (k, Na, La))
        answer_ids = answer_ids.to(torch.int64).contiguous()
        answer_atts = answer_atts.to(torch.int64).contiguous()
        question_states = question_states.contiguous()
        start_ids = answer_ids[0, 0].repeat(B, 1)
        h0 = dec(start_ids, encoder_hidden_states=question_states, encoder_attention_mask=question_atts).last_hidden_state
        logits0 = dec.head_logits(K.cast_bf16(h0.reshape(B, Hd)))                                  # [B, Vp]
        first_tok = answer_ids[:, 1].to(torch.int32).contiguous()
        S = B * k
        if fused:
            vals, ids = K.answer_topk(logits0, V, first_tok, k)
        if not fused or stage1_ids is not None or want_traces:
            logp_first = torch.log_softmax(logits0[:, :V], -1).index_select(1, first_tok.long())
        if not fused:
            order = torch.sort(logp_first, dim=1, descending=True, stable=True).indices[:, :k]     # lowest candidate first among equals
            vals, ids = torch.gather(logp_first, 1, order).contiguous(), order.to(torch.int32).contiguous()
        if stage1_ids is not None:
            ids = torch.as_tensor(stage1_ids, device=dev).reshape(B, k).to(torch.int32).contiguous()
            vals = torch.gather(logp_first, 1, ids.long()).contiguous()
        if fused:
            input_ids, labels, kv_idx, mask2d = K.vqa_candidates(answer_ids, answer_atts, ids, self.pad_token_id)
            atts = None
        else:
            flat = ids.reshape(S).long()
            input_ids = answer_ids.index_select(0, flat)
            atts = answer_atts.index_select(0, flat)
            labels = input_ids[:, 1:].masked_fill(input_ids[:, 1:] == self.pad_token_id, -100).contiguous()
            kv_idx = (torch.arange(S, device=dev, dtype=torch.int32) // k).contiguous()
            mask2d = None
        row_atts = question_atts.index_select(0, kv_idx.long())
        h = dec(input_ids, attention_mask=atts, encoder_hidden_states=question_states, encoder_attention_mask=row_atts, kv_idx=kv_idx,
                self_mask2d=mask2d).last_hidden_state                                               # [S, La, Hd]
        cache = self.__dict__.setdefault("_scored_rows", {})
        rows = cache.get((S, La, dev))
        if rows is None:
            rows = (torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(1) * La
                    + torch.arange(La - 1, device=dev, dtype=torch.int32)).reshape(-1).contiguous()
            cache[(S, La, dev)] = rows
        _, hb = K.gather_rows(h.reshape(S * La, Hd), rows, Hd, want_f32=False, want_bf16=True)
        flat_labels = labels.reshape(-1)
        if fused:
            loss_rows, _ = dec.head_loss_rows(hb, flat_labels)
            loss_rows = loss_rows.reshape(S, La - 1).contiguous()
            topk_probs, topk_ids, scores = K.vqa_rerank(loss_rows, vals, ids)
        else:
            z = dec.head_logits(hb)[:, :V]
            picked = torch.gather(z, 1, flat_labels.clamp(min=0).unsqueeze(1)).squeeze(1)
            loss_rows = torch.where(flat_labels >= 0, torch.logsumexp(z, -1) - picked, torch.zeros_like(picked)).reshape(S, La - 1)
            scores = vals - loss_rows.sum(1).reshape(B, k)
            order = torch.sort(scores, dim=1, descending=True, stable=True).indices
            topk_probs = torch.gather(torch.softmax(scores, -1), 1, order)
            topk_ids = torch.gather(ids, 1, order)
        out = (topk_ids.long(), topk_probs)
        if want_traces:
            out += (dict(logits0=logits0[:, :V], logp_first=logp_first, stage1_logp=vals, stage1_ids=ids, loss_rows=loss_rows, scores=scores),)
        return out
