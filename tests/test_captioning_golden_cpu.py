"""Captioning fine-tune, float64 restatement pinned to the reference's golden (tests/golden/<case>_captioning.npz, written by
make_golden_captioning.py from the REAL reference XVLMForMLMCaptioning on CPU fp32): the 2-D-masked BERT encoder with explicit position ids
and cross-attention, the MLM head at the masked slots, and the label-smoothed, weight-normalised KL loss, composed from oracle.x2vlm_oracle
pieces plus the captioning parts written out here.  Loss, prediction scores and gradient norms / samples, both collate forms, tiny and
base_shallow (V = 30522, L = 58).

Bounds (float64 against the reference's fp32; measured worst in brackets): loss 1e-5 relative [3e-7]; scores 1e-4 of max-abs [3e-6];
gradient norms 1e-4 relative [2e-6]; gradient samples 1e-3 of the tensor's max-abs sample [2e-5]."""
import importlib

import numpy as np
import pytest
import torch

from cases import CASES
from cases_captioning import CAP_CASES, GRAD_SAMPLE, LABEL_SMOOTHING, SCORE_COLS
from oracle import x2vlm_oracle as O

GOLD_DIR = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden")


def gold(name):
    return np.load("%s/%s_captioning.npz" % (GOLD_DIR, name))


def ignore_id(case):
    return 101 if CASES[case]["vocab"] > 2000 else 1


def smoothed_loss(scores, labels, w, V, ignore, ls):
    """LabelSmoothingLoss (model_generation.py:16-51) + loss_mask_and_normalize, restated."""
    z = scores.reshape(-1, V)
    labels, w = labels.reshape(-1), w.reshape(-1).to(z.dtype)
    q = torch.full(z.shape, ls / (V - 2), dtype=z.dtype)
    q[:, ignore] = 0
    q.scatter_(1, labels.view(-1, 1), 1.0 - ls)
    q[labels == ignore] = 0
    logp = torch.log_softmax(z, -1)
    kl = torch.where(q > 0, q * (torch.log(q.clamp_min(1e-300)) - logp), torch.zeros_like(q)).sum(-1)
    return (kl * w / (w.sum() + 1e-5)).sum()


def captioning_forward(sd, cfg, d, ignore, ls):
    """image -> vision tower (oracle); text: word + pos[position_ids] + type0, LayerNorm; every layer's self-attention under the
    [B, L, L] additive mask (1 - m) * -10000 (xbert get_extended_attention_mask, 3-D branch); fusion layers attend the image tokens;
    MLM head at masked_pos; smoothed loss."""
    image_embeds = O.vision_encoder(sd, cfg, d["image"].double())
    p = "text_encoder.bert.embeddings."
    e = sd[p + "word_embeddings.weight"][d["text_ids_masked"]] + sd[p + "token_type_embeddings.weight"][0] \
        + sd[p + "position_embeddings.weight"][d["position_ids"]]
    h = O.layer_norm(e, sd[p + "LayerNorm.weight"], sd[p + "LayerNorm.bias"], 1e-12)
    self_mask = (1.0 - d["text_atts"].double())[:, None, :, :] * -10000.0
    enc_mask = torch.zeros(image_embeds.shape[0], 1, 1, image_embeds.shape[1], dtype=torch.float64)
    for i in range(cfg.text_layers):
        h = O.bert_layer(sd, cfg, i, h, self_mask, image_embeds, enc_mask)
    scores = O.mlm_logits_from_hidden(sd, h, d["masked_pos"])
    return smoothed_loss(scores, d["masked_ids"], d["masked_weight"], cfg.vocab, ignore, ls), scores


@pytest.mark.parametrize("name", list(CAP_CASES))
@pytest.mark.parametrize("form", ["plain", "fgfree"])
def test_float64_restatement_matches_reference_golden(synthetic, name, form):
    cc = CAP_CASES[name]
    c = CASES[cc["case"]]
    g = gold(name)
    cfg = O.config_from_case(c)
    sd = {k: v.double().detach().requires_grad_(True) for k, v in O.make_params(cfg, cc["wseed"], synthetic.synth_tensor).items()}
    d = synthetic.synth_captioning_batch(cc["bseed"], cc["batch"], cc["max_tokens"], cc["max_masks"], c["image_res"], c["vocab"],
                                         fg_free=form == "fgfree")
    loss, scores = captioning_forward(sd, cfg, d, ignore_id(cc["case"]), LABEL_SMOOTHING)
    loss.backward()
    ref = float(g[form + "_loss"])
    assert abs(float(loss.detach()) - ref) <= 1e-5 * max(1.0, abs(ref)), (float(loss.detach()), ref)
    s = scores.detach()
    if form + "_scores" in g:
        want = torch.from_numpy(g[form + "_scores"]).double()
        assert float((s - want).abs().max()) <= 1e-4 * float(want.abs().max())
    else:
        want = torch.from_numpy(g[form + "_scores_cols"]).double()
        assert float((s[:, :, SCORE_COLS] - want).abs().max()) <= 1e-4 * float(want.abs().max())
        assert float((torch.logsumexp(s, -1) - torch.from_numpy(g[form + "_scores_lse"])).abs().max()) <= 1e-4 * float(want.abs().max())
    names = list(g["param_names"])
    for key, pname in GRAD_SAMPLE.items():
        gr = sd[pname].grad.reshape(-1)
        norm_ref = float(g[form + "_grad_norms"][names.index(pname)])
        assert abs(float(gr.norm()) - norm_ref) <= 1e-4 * norm_ref, (pname, float(gr.norm()), norm_ref)
        idx = torch.arange(64) * (gr.numel() - 1) // 63
        ws = torch.from_numpy(g[form + "_grad_" + key]).double()
        assert float((gr[idx] - ws).abs().max()) <= 1e-3 * float(ws.abs().max()), pname
