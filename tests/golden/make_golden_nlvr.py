#!/usr/bin/env python3
"""Golden vectors for NLVR2: the REAL reference model's XVLMForNLVR (models/model_classification.py) on CPU fp32 in eval mode, seeded synthetic
weights, the case's batch of cases_nlvr.nlvr_batch.  Build container only.

Recorded per case:
  logits [B, 2], loss                              forward(image, text_ids, text_atts, targets, train=False / train=True)
  total_grad_norm, gradnorm/<param>                float64 norms of d(loss)
  targets [B], pred [B], acc                       the targets used; the reference's own `_, pred_class = prediction.max(1)` and
                                                   `(targets == pred_class).sum() / targets.size(0)` lines (NLVR.py:88-89)
  logit_margin                                     cases_nlvr.logit_margin of the logits
  sd_names, sd_shapes, init_params                 the model's sorted state_dict names and shapes, its init_params
and, in tiny_nlvr.npz:
  map_pairs [n, 2]                                 (key handed to load_state_dict, checkpoint key its tensor came from) for every non-vision key
                                                   the reference's load_pretrained(is_eval=False) produces from cases_nlvr.pretrain_state

The reference's forward calls F.cross_entropy without ignore_index, whose default is the -100 that XVLMForClassification passes explicitly: the
tiny_ignore case runs the same line.

Asserted: every parameter receives a gradient; logit_margin >= cases_nlvr.MARGIN (a bf16 error in the logits below half of it cannot flip an
argmax).

writes tests/golden/<case>_nlvr.npz for NLVR_CASES
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import reference_shims  # noqa: E402
from cases_nlvr import MARGIN, NLVR_CASES, logit_margin, nlvr_batch, nlvr_config, pretrain_state  # noqa: E402

synthetic = importlib.import_module("x2-vlm_amd.synthetic")


def build(name):
    from models.model_classification import XVLMForNLVR
    cfg = nlvr_config(name, "/tmp/x2golden_nlvr_%s" % name)
    return XVLMForNLVR(config=cfg), cfg


def grad_norms(model, loss):
    model.zero_grad(set_to_none=True)
    loss.backward()
    norms = {}
    for n, p in model.named_parameters():
        assert p.grad is not None, "no gradient for " + n
        norms[n] = float(p.grad.double().norm())
    return norms, sum(v * v for v in norms.values()) ** 0.5


def recorded_mapping(name):
    """what the reference's load_pretrained hands to load_state_dict for the synthetic pre-training checkpoint: (key, source key) pairs"""
    mp = importlib.import_module("x2-vlm_amd.model_pretrain")           # parameter names and shapes of the pre-training model (== the reference's)
    model, cfg = build(name)
    pre = mp.XVLM(config=dict(cfg), load_vision_params=False, load_text_params=False)
    state = pretrain_state(synthetic, [(n, tuple(t.shape)) for n, t in pre.state_dict().items() if t.is_floating_point()])
    finger = {t.numpy().tobytes(): n for n, t in state.items()}
    assert len(finger) == len(state)
    ckpt = "/tmp/x2golden_nlvr_%s/pretrain.th" % name
    torch.save({"model": state}, ckpt)
    seen = {}
    real = model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: (seen.update(sd), real(sd, strict=strict))[1]
    model.load_pretrained(ckpt, cfg, is_eval=False)
    pairs = sorted((key, finger[t.numpy().tobytes()]) for key, t in seen.items() if not key.startswith("vision_encoder."))
    assert any(k.startswith("text_encoder.encoder.layer.") for k, _ in pairs) and not any(k.startswith("cls_head.") for k, _ in pairs)
    return pairs


def run_case(name):
    nc = NLVR_CASES[name]
    model, _ = build(name)
    synthetic.synth_state_dict(model, nc["wseed"])
    model.eval()
    b = nlvr_batch(synthetic, name)
    loss = model(b["image"], b["text_ids"], b["text_atts"], targets=b["targets"], train=True)
    norms, total = grad_norms(model, loss)
    with torch.no_grad():
        prediction = model(b["image"], b["text_ids"], b["text_atts"], targets=b["targets"], train=False)
    _, pred_class = prediction.max(1)
    accuracy = (b["targets"] == pred_class).sum() / b["targets"].size(0)
    margin = logit_margin(prediction.numpy())
    assert margin >= MARGIN, "%s: logit margin %.4f < %.4f" % (name, margin, MARGIN)
    sd = sorted((n, tuple(t.shape)) for n, t in model.state_dict().items())
    out = dict(logits=prediction.numpy(), loss=np.array(float(loss)), total_grad_norm=np.array(total), targets=b["targets"].numpy(),
               pred=pred_class.numpy(), acc=np.array(accuracy.item()), logit_margin=np.array(margin),
               sd_names=np.array([n for n, _ in sd]), sd_shapes=np.array([",".join(map(str, s)) for _, s in sd]),
               init_params=np.array(list(model.init_params), dtype=str))
    for n, v in norms.items():
        out["gradnorm/" + n] = np.array(v)
    if name == "tiny":
        out["map_pairs"] = np.array(recorded_mapping(name))
    path = os.path.join(HERE, "%s_nlvr.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote %s (%d bytes): loss %.6f, grad norm %.5f, logit margin %.4f, accuracy %.4f"
          % (path, os.path.getsize(path), float(loss), total, margin, accuracy.item()))


def main():
    reference_shims.install()
    reference_shims.ensure_process_group()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(NLVR_CASES)):
        run_case(name)


if __name__ == "__main__":
    main()
