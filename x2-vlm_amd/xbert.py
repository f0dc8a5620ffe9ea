"""BERT text / fusion encoder with the reference's module tree and state-dict keys
(models/xbert.py), executed by the HIP stages EmbeddingsFn / BertLayersFn / MlmLossFn.
Layers >= config.fusion_layer carry a cross-attention sub-block; `mode` selects the layer range
(xbert.py:674-686).  nn.Modules here are parameter containers only.
"""
import json
import os
from types import SimpleNamespace

import torch
import torch.nn as nn

from . import kernels as K
from . import ops
from .engine import BertLayersFn, EmbeddingsFn, MlmLossFn, SeqLmLossFn, _mask_pad, bert_layer_param_names, lm_head_transform


_FIXED_SEEDS = []


def _key_mask(atts, neg):
    """0/1 attention mask [S, L] -> additive fp32 key mask (1 - m) * neg in the attention kernels' padded layout."""
    if atts.is_cuda and atts.dtype == torch.int64:
        return K.additive_mask(atts.contiguous(), neg)
    return _mask_pad((1.0 - atts.float()) * neg, atts.shape[1])


def _text_masks(atts):
    """(self_mask, self_mask2d) of a text attention mask: [S, L] -> additive key mask; [S, L, L] (the captioning collate's tril / FG-free
    mask, applied per (query, key) as the reference's get_extended_attention_mask does) -> the 2-D additive mask of attn_fwd_mask2d."""
    if atts.dim() == 3:
        return None, K.additive_mask2d(atts.to(torch.int64).contiguous(), -10000.0)
    return _key_mask(atts, -10000.0), None


def next_dropout_seed():
    """Per-call dropout seed from the host RNG (torch.manual_seed governs it; no device sync).
    Tests push explicit seeds onto _FIXED_SEEDS."""
    if _FIXED_SEEDS:
        return _FIXED_SEEDS.pop(0)
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


class BertConfig:
    """The handful of fields of HF's BertConfig this path reads (config.json of the text encoder dir)."""
    _defaults = dict(vocab_size=30522, hidden_size=768, num_hidden_layers=12, num_attention_heads=12,
                     intermediate_size=3072, hidden_act="gelu", hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, max_position_embeddings=512, type_vocab_size=2,
                     initializer_range=0.02, layer_norm_eps=1e-12, pad_token_id=0)

    def __init__(self, **kw):
        for k, v in dict(self._defaults, **kw).items():
            setattr(self, k, v)

    @classmethod
    def from_json_file(cls, path):
        with open(path) as f:
            return cls(**json.load(f))


class BertEmbeddings(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.word_embeddings = nn.Embedding(config.vocab_size, config.hidden_size, padding_idx=config.pad_token_id)
        self.position_embeddings = nn.Embedding(config.max_position_embeddings, config.hidden_size)
        self.token_type_embeddings = nn.Embedding(config.type_vocab_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)
        self.register_buffer("position_ids", torch.arange(config.max_position_embeddings).expand((1, -1)))
        self.eps = config.layer_norm_eps
        self.config = config

    def forward(self, input_ids, position_ids=None):
        """position_ids: None (positions 0 .. L-1) or int (S, L) / (1, L) explicit positions, repeats allowed (xbert.py:189-216)."""
        drop = K.NO_DROP
        if self.training and self.config.hidden_dropout_prob > 0:
            drop = K.dropout_spec(self.config.hidden_dropout_prob, next_dropout_seed(), 1000)
        args = (input_ids, self.eps, drop, self.word_embeddings.weight, self.position_embeddings.weight,
                self.token_type_embeddings.weight, self.LayerNorm.weight, self.LayerNorm.bias)
        if position_ids is None:
            return EmbeddingsFn.apply(*args)
        return EmbeddingsFn.apply(*args, position_ids)


class BertSelfAttention(nn.Module):
    def __init__(self, config, is_cross_attention):
        super().__init__()
        kin = config.encoder_width if is_cross_attention else config.hidden_size
        self.query = nn.Linear(config.hidden_size, config.hidden_size)
        self.key = nn.Linear(kin, config.hidden_size)
        self.value = nn.Linear(kin, config.hidden_size)


class BertSelfOutput(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)


class BertAttention(nn.Module):
    def __init__(self, config, is_cross_attention=False):
        super().__init__()
        self.self = BertSelfAttention(config, is_cross_attention)
        self.output = BertSelfOutput(config)


class BertIntermediate(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.intermediate_size)


class BertOutput(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.intermediate_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)


class BertLayer(nn.Module):
    def __init__(self, config, layer_num):
        super().__init__()
        self.attention = BertAttention(config)
        self.has_cross_attention = layer_num >= config.fusion_layer
        if self.has_cross_attention:
            self.crossattention = BertAttention(config, is_cross_attention=True)
        self.intermediate = BertIntermediate(config)
        self.output = BertOutput(config)


_IDENTITY_CSR = {}      # (rows, device) -> (kv_idx, seq_off, seq_ids) of the identity row -> image map


class BertEncoder(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.layer = nn.ModuleList([BertLayer(config, i) for i in range(config.num_hidden_layers)])

    def run(self, hidden, text_atts, enc=None, enc_atts=None, mode="multi_modal", kv_idx=None, self_mask2d=None):
        """hidden (S,L,Hd) fp32; enc (Bi,T,Dv) image tokens shared through kv_idx (int (S,), None = identity);
        enc_atts (S,T) per text row; text_atts (S,L) per key or (S,L,L) per (query, key); self_mask2d: the additive fp32
        [S, L, round_up(L, 64)] mask already in attn_fwd_mask2d's layout (kernels.vqa_candidates), taking text_atts' place."""
        cfg = self.config
        lo, hi = {"text": (0, cfg.fusion_layer), "fusion": (cfg.fusion_layer, cfg.num_hidden_layers),
                  "multi_modal": (0, cfg.num_hidden_layers)}[mode]
        S, L, _ = hidden.shape
        drop = None
        if self.training and (cfg.hidden_dropout_prob > 0 or cfg.attention_probs_dropout_prob > 0):
            drop = dict(seed=next_dropout_seed(), p_hidden=cfg.hidden_dropout_prob, p_attn=cfg.attention_probs_dropout_prob)
        meta = dict(lo=lo, hi=hi, fusion_at=cfg.fusion_layer, heads=cfg.num_attention_heads, eps=cfg.layer_norm_eps,
                    self_mask=None, self_mask2d=None, enc_mask=None, kv_idx=None,
                    seq_off=None, seq_ids=None, drop=drop)
        if self_mask2d is not None:
            assert self_mask2d.dtype == torch.float32 and self_mask2d.shape == (S, L, K.round_up(L, 64)) and self_mask2d.is_contiguous()
            meta["self_mask2d"] = self_mask2d
        else:
            meta["self_mask"], meta["self_mask2d"] = _text_masks(text_atts)
        cross = enc is not None and hi > cfg.fusion_layer
        if cross:
            Bi = enc.shape[0]
            # transformers 4.12.5 invert_attention_mask, fp32 branch: (1 - m) * -1e9
            meta["enc_mask"] = _key_mask(enc_atts, -1e9)
            if kv_idx is None:
                assert Bi == S, "encoder batch %d != text batch %d and no kv_idx given" % (Bi, S)
                if enc.is_cuda and torch.is_grad_enabled() and (hidden.requires_grad or enc.requires_grad or self.training) \
                        and K.attn_bwd_form(L, enc.shape[1], shared_kv=True) == 2:
                    # one text row per image (predict_bbox: xvlm.py:905-915) as the identity sharing: the backward then runs as ONE
                    # kernel per layer (attn_bwd_onepass_grouped_kernel, a workgroup per (image, head)) instead of the per-row dQ and
                    # (only when a backward will follow: inference keeps kv_idx None and with it the forward's walk / resident kernels)
                    # dK/dV kernels - and the tail segment needs no second stream (engine.AUX.auto)
                    ident = _IDENTITY_CSR.get((S, enc.device))
                    if ident is None:
                        ar = torch.arange(S + 1, device=enc.device, dtype=torch.int32)
                        ident = (ar[:S].contiguous(), ar, ar[:S].contiguous())
                        if not torch.cuda.is_current_stream_capturing():      # a tensor born inside a capture belongs to that graph's pool
                            _IDENTITY_CSR[(S, enc.device)] = ident
                    meta.update(kv_idx=ident[0], seq_off=ident[1], seq_ids=ident[2])
            else:
                kv = kv_idx.to(torch.int32).contiguous()
                if kv.is_cuda:
                    off, order = K.kv_csr(kv, Bi)          # one launch: kv changes every step with the sampled negatives
                else:
                    order = torch.argsort(kv, stable=True).to(torch.int32).contiguous()
                    off = torch.zeros(Bi + 1, device=kv.device, dtype=torch.int32)
                    off[1:] = torch.cumsum(torch.bincount(kv, minlength=Bi), 0)
                meta.update(kv_idx=kv, seq_off=off, seq_ids=order)
        cache = self.__dict__.setdefault("_param_lists", {})      # see beit2.VisionTransformer._params
        params = cache.get((lo, hi, cross))
        if params is None:
            sd = dict(self.named_parameters())
            params = cache[(lo, hi, cross)] = [sd[n] for n in bert_layer_param_names(lo, hi, cfg.fusion_layer, cross)]
        return BertLayersFn.apply(hidden, enc if cross else None, meta, *params)


class BertModel(nn.Module):
    def __init__(self, config, add_pooling_layer=False):
        super().__init__()
        assert not add_pooling_layer
        self.config = config
        self.embeddings = BertEmbeddings(config)
        self.encoder = BertEncoder(config)
        self.apply(lambda m: _bert_init(m, config.initializer_range))

    def get_input_embeddings(self):
        return self.embeddings.word_embeddings

    def forward(self, input_ids=None, attention_mask=None, encoder_embeds=None, encoder_hidden_states=None,
                encoder_attention_mask=None, return_dict=True, mode="multi_modal", kv_idx=None, position_ids=None, self_mask2d=None,
                **unused):
        """xbert.py:1075-1220 (encoder path: no decoder cache, no head masks).  attention_mask (S,L) or (S,L,L), or the prebuilt
        additive self_mask2d of BertEncoder.run in its place."""
        _refuse_unused("BertModel", unused)
        hidden = self.embeddings(input_ids, position_ids) if encoder_embeds is None else encoder_embeds
        S, L = hidden.shape[:2]
        if attention_mask is None and self_mask2d is None:
            attention_mask = torch.ones(S, L, device=hidden.device)
        if encoder_hidden_states is not None and encoder_attention_mask is None:
            encoder_attention_mask = torch.ones(S, encoder_hidden_states.shape[1], device=hidden.device)
        out = self.encoder.run(hidden, attention_mask, encoder_hidden_states, encoder_attention_mask, mode, kv_idx, self_mask2d)
        return SimpleNamespace(last_hidden_state=out) if return_dict else (out,)


class BertPredictionHeadTransform(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.dense = nn.Linear(config.hidden_size, config.hidden_size)
        self.LayerNorm = nn.LayerNorm(config.hidden_size, eps=config.layer_norm_eps)


class BertLMPredictionHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.transform = BertPredictionHeadTransform(config)
        self.decoder = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.bias = nn.Parameter(torch.zeros(config.vocab_size))


class BertOnlyMLMHead(nn.Module):
    def __init__(self, config):
        super().__init__()
        self.predictions = BertLMPredictionHead(config)


class LMHeadRows:
    """The LM head `cls` (transform + decoder tied to the word embeddings of `bert`) of the two models that carry one: its parameters as the
    engine takes them, and the head applied to gathered bf16 rows at inference."""

    def head_params(self):
        """(eps, dense weight, dense bias, LayerNorm weight, LayerNorm bias, decoder bias, tied word embeddings): the head as
        engine.lm_head_transform and the two loss Functions take it"""
        pr = self.cls.predictions
        return (self.config.layer_norm_eps, pr.transform.dense.weight, pr.transform.dense.bias, pr.transform.LayerNorm.weight,
                pr.transform.LayerNorm.bias, pr.bias, self.bert.embeddings.word_embeddings.weight)

    def _head(self, rows):
        """-> (transformed bf16 rows [R, Hd], padded bf16 embeddings [Vp, Hd], padded bias [Vp]) of bf16 hidden rows [R, Hd]"""
        tb, _, _, _, _, Eb, _, bias_p = lm_head_transform(rows, *self.head_params())
        return tb, Eb, bias_p

    def head_logits(self, rows):
        """fp32 logits [R, Vp] of bf16 hidden rows [R, Hd] (Vp = the vocabulary rounded up to 64; the padding columns hold the zero-padded
        decoder's output and mean nothing)"""
        tb, Eb, bias = self._head(rows)
        return K.gemm_nt(tb, Eb, bias=bias, out_dtype=torch.float32)

    def head_loss_rows(self, rows, labels):
        """(loss_row [R] = logsumexp - logit of the label, 0 where the label is negative; lse [R]) of bf16 hidden rows [R, Hd], the
        logits staying in the GEMM (kernels.mlm_ce_rows)"""
        tb, Eb, bias = self._head(rows)
        return K.mlm_ce_rows(tb, Eb, bias, labels, self.config.vocab_size)


class BertForMaskedLM(nn.Module, LMHeadRows):
    """xbert.py:1567-1673.  decoder.weight is tied to the word embeddings (HF tie_weights)."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.bert = BertModel(config)
        self.cls = BertOnlyMLMHead(config)
        self.apply(lambda m: _bert_init(m, config.initializer_range))
        self.cls.predictions.decoder.weight = self.bert.embeddings.word_embeddings.weight

    def mlm_loss_from_hidden(self, sequence_output, masked_pos, labels, keep_logits=False):
        """gather masked positions (xbert.py:1588-1589), head, CE.  Returns (loss, lse [B*M], logits [B*M, Vp] or None: the
        logits only exist when asked for - the loss comes from softmax statistics reduced inside the decoder GEMM)."""
        B, L, Hd = sequence_output.shape
        flat = (torch.arange(B, device=masked_pos.device).unsqueeze(1) * L + masked_pos).reshape(-1)
        rows = ops.gather_rows(sequence_output.reshape(B * L, Hd), flat)
        pr = self.cls.predictions
        return MlmLossFn.apply(rows, labels, self.config.layer_norm_eps, keep_logits, pr.transform.dense.weight, pr.transform.dense.bias,
                               pr.transform.LayerNorm.weight, pr.transform.LayerNorm.bias, pr.bias,
                               self.bert.embeddings.word_embeddings.weight)

    def smoothed_mlm_loss_from_hidden(self, sequence_output, masked_pos, labels, weights, ignore_index, label_smoothing, keep_logits=False):
        """mlm_loss_from_hidden with the captioning fine-tune's loss: label-smoothed KL per masked slot (ignore_index gets no mass, slots
        labelled with it no loss), weighted by weights / (sum(weights) + 1e-5) and summed (model_generation.py LabelSmoothingLoss +
        loss_mask_and_normalize).  Returns (loss, lse, logits or None) as mlm_loss_from_hidden."""
        B, L, Hd = sequence_output.shape
        flat = (torch.arange(B, device=masked_pos.device).unsqueeze(1) * L + masked_pos).reshape(-1)
        rows = ops.gather_rows(sequence_output.reshape(B * L, Hd), flat)
        w = weights.reshape(-1).to(torch.float32).contiguous()
        head = self.head_params()
        return MlmLossFn.apply(rows, labels, head[0], keep_logits, *head[1:], (w, int(ignore_index), float(label_smoothing)))

    def forward(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None,
                labels=None, return_dict=True, mode="multi_modal", masked_pos=None, return_logits=False, position_ids=None, **unused):
        _refuse_unused("BertForMaskedLM", unused)
        if masked_pos is None:
            raise NotImplementedError("need check!")     # same as the reference, xbert.py:1650-1651
        h = self.bert(input_ids, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                      encoder_attention_mask=encoder_attention_mask, mode=mode, position_ids=position_ids).last_hidden_state
        lab = labels if labels is not None else torch.full_like(masked_pos, -100)
        loss, _, logits = self.mlm_loss_from_hidden(h, masked_pos, lab, keep_logits=return_logits)
        if logits is not None:
            logits = logits[:, :self.config.vocab_size].view(masked_pos.shape[0], masked_pos.shape[1], -1)
        if return_logits:
            return logits
        return SimpleNamespace(loss=loss if labels is not None else None, logits=logits)


class BertLMHeadModel(nn.Module, LMHeadRows):
    """xbert.py:1268-1400, the causal answer decoder of XVLMForVQA: `bert` with cross-attention in every layer (config.fusion_layer = 0,
    config.encoder_width = the question states' width) and the LM head `cls`, whose decoder.weight is tied to ITS OWN word embeddings.
    forward returns the hidden states of a causal pass and, with labels, the next-token LM loss formed inside the decoder GEMM (HIP tensors
    only; label smoothing and return_logits are refused); head_logits / head_loss_rows apply the head to gathered rows at inference."""

    def __init__(self, config, label_smoothing=0.0):
        super().__init__()
        self.config = config
        self.label_smoothing = label_smoothing
        self.bert = BertModel(config)
        self.cls = BertOnlyMLMHead(config)
        self.apply(lambda m: _bert_init(m, config.initializer_range))
        self.cls.predictions.decoder.weight = self.bert.embeddings.word_embeddings.weight
        self.cls.predictions.decoder.bias = self.cls.predictions.bias      # one parameter under both names, as the reference serialises it

    def get_output_embeddings(self):
        return self.cls.predictions.decoder

    def forward(self, input_ids=None, attention_mask=None, encoder_hidden_states=None, encoder_attention_mask=None, labels=None, return_dict=True,
                is_decoder=True, reduction="mean", mode="multi_modal", kv_idx=None, self_mask2d=None, _next_labels=None, _seq_weights=None,
                **unused):
        """-> last_hidden_state [S, L, Hd] of the causal pass.  The self-attention mask is tril x attention_mask [S, L] (None: ones), or
        the additive self_mask2d kernels.vqa_candidates / vqa_train_rows built from the same rule; encoder_hidden_states [Bq, T, Hd] may be
        shared by several rows through kv_idx, encoder_attention_mask is per row [S, T].

        labels int64 [S, L], -100 where ignored (xbert.py:1373-1387): position t is scored against labels[:, t + 1], t = 0 .. L - 2, and the
        result also carries .loss - reduction='none': fp32 [S], the sum over a row's scored positions, differentiable for any cotangent;
        reduction='mean': the mean over the non-ignored tokens (NaN when there is none, as CrossEntropyLoss gives).  The logits are never stored;
        return_dict=False gives (loss, last_hidden_state).
        Not part of the mirrored signature (XVLMForVQA's training step): _next_labels int64 [S, L - 1], the already shifted labels in labels'
        place; _seq_weights fp32 [S] adds .total = sum_s _seq_weights[s] * loss[s], then THE differentiable output (.loss carries no gradient)."""
        _refuse_unused("BertLMHeadModel", unused)
        if not is_decoder:
            raise NotImplementedError("BertLMHeadModel.forward(is_decoder=False) is not supported by the HIP path")
        with_loss = labels is not None or _next_labels is not None
        if with_loss:
            ops.require_hip(input_ids, "BertLMHeadModel.forward(labels=...): the LM loss")
            if self.label_smoothing > 0:
                raise NotImplementedError("BertLMHeadModel.forward(labels=...) with label_smoothing > 0 is not implemented (the smoothed head "
                                          "is the captioning model's)")
            if reduction not in ("mean", "none"):
                raise ValueError("BertLMHeadModel.forward: reduction=%r (mean or none)" % (reduction,))
        S, L = input_ids.shape
        if with_loss and L < 2:
            raise ValueError("BertLMHeadModel.forward(labels=...): %d position leaves no next token to score" % L)
        if self_mask2d is None and L > 1:
            atts = torch.ones(S, L, dtype=torch.long, device=input_ids.device) if attention_mask is None else attention_mask.long()
            attention_mask = torch.tril(torch.ones(L, L, dtype=torch.long, device=input_ids.device)).unsqueeze(0) * atts.unsqueeze(1)
        h = self.bert(input_ids, attention_mask=attention_mask, encoder_hidden_states=encoder_hidden_states,
                      encoder_attention_mask=encoder_attention_mask, mode=mode, kv_idx=kv_idx, self_mask2d=self_mask2d).last_hidden_state
        if not with_loss:
            return SimpleNamespace(last_hidden_state=h) if return_dict else (h,)
        nxt = _next_labels if _next_labels is not None else labels[:, 1:]
        nxt = nxt.to(torch.int64).reshape(-1).contiguous()
        rows = ops.gather_rows(h.reshape(S * L, -1), self._scored_rows(S, L, h.device))
        head = self.head_params()
        total = None
        if reduction == "none" or _seq_weights is not None:
            loss, total = SeqLmLossFn.apply(rows, nxt, L - 1, _seq_weights, *head)
        else:
            loss = MlmLossFn.apply(rows, nxt, head[0], False, *head[1:])[0]
        if not return_dict:
            return (loss, h)
        return SimpleNamespace(loss=loss, total=total, last_hidden_state=h)

    def _scored_rows(self, S, L, dev):
        """int32 [S * (L - 1)]: the flat positions 0 .. L - 2 of every row of [S, L]"""
        cache = self.__dict__.setdefault("_scored_rows_idx", {})
        rows = cache.get((S, L, dev))
        if rows is None:
            rows = (torch.arange(S, device=dev, dtype=torch.int32).unsqueeze(1) * L
                    + torch.arange(L - 1, device=dev, dtype=torch.int32)).reshape(-1).contiguous()
            if not torch.cuda.is_current_stream_capturing():          # a tensor born inside a capture belongs to that graph's pool
                cache[(S, L, dev)] = rows
        return rows


def _refuse_unused(who, unused):
    """keyword arguments of the reference's signature this path does not implement raise instead of vanishing"""
    for k, v in unused.items():
        if isinstance(v, torch.Tensor) or v not in (None, False):
            raise NotImplementedError("%s.forward(%s=...) is not supported by the HIP path" % (who, k))


def _bert_init(m, std):
    if isinstance(m, (nn.Linear, nn.Embedding)):
        m.weight.data.normal_(mean=0.0, std=std)
    elif isinstance(m, nn.LayerNorm):
        m.bias.data.zero_()
        m.weight.data.fill_(1.0)
    if isinstance(m, nn.Linear) and m.bias is not None:
        m.bias.data.zero_()


def get_bert_config(encoder_rpath, num_hidden_layers=12, cross_start_at=12):
    """xvlm.py:122-137."""
    config = BertConfig.from_json_file(os.path.join(encoder_rpath, "config.json"))
    config.num_hidden_layers = num_hidden_layers
    config.fusion_layer = cross_start_at
    config.embedding_dim = config.hidden_size
    return config
