#!/usr/bin/env python3
"""Golden vectors for the captioning fine-tune: the REAL reference model (models/model_generation.py: XVLMForMLMCaptioning) on CPU fp32,
seeded synthetic weights and seeded captioning batches (x2-vlm_amd/synthetic.py synth_captioning_batch) in both collate forms, plain (tril)
and FG-free.  The reference builds a BertTokenizer from the text-encoder directory: this script writes a vocab.txt there whose size is the
case's vocabulary and whose [CLS] / [SEP] / [MASK] ids are the ones the synthetic batches use.  Build container only.

writes tests/golden/<case>_captioning.npz for CAP_CASES
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
from cases import CASES  # noqa: E402
from cases_captioning import CAP_CASES, GRAD_SAMPLE, SCORE_COLS, caption_config, write_vocab  # noqa: E402

synthetic = importlib.import_module("x2-vlm_amd.synthetic")


def bert_tokenizer(path, *a, **k):
    from transformers import BertTokenizer
    return BertTokenizer(os.path.join(path, "vocab.txt"), do_lower_case=True)


def run_case(name):
    cc = CAP_CASES[name]
    c = CASES[cc["case"]]
    workdir = "/tmp/x2golden_cap_%s" % name
    cfg = caption_config(cc["case"], workdir)
    write_vocab(cfg["text_encoder"], c["vocab"])
    from models.model_generation import XVLMForMLMCaptioning
    model = XVLMForMLMCaptioning(config=cfg)
    assert model.tokenizer.cls_token_id == cfg["cls_token_id"] and model.tokenizer.vocab_size == c["vocab"]
    synthetic.synth_state_dict(model, cc["wseed"])
    model.eval()
    out = {}
    names = [n for n, _ in model.named_parameters()]
    for form, fg in (("plain", False), ("fgfree", True)):
        d = synthetic.synth_captioning_batch(cc["bseed"], cc["batch"], cc["max_tokens"], cc["max_masks"], c["image_res"], c["vocab"], fg_free=fg)
        args = (d["image"], d["text_ids_masked"], d["text_atts"], d["position_ids"], d["masked_pos"], d["masked_ids"], d["masked_weight"])
        for p in model.parameters():
            p.grad = None
        loss = model(*args)
        loss.backward()
        with torch.no_grad():
            image_embeds, image_atts = model.get_vision_embeds(d["image"])
            scores = model.text_encoder(d["text_ids_masked"], attention_mask=d["text_atts"], position_ids=d["position_ids"],
                                        encoder_hidden_states=image_embeds, encoder_attention_mask=image_atts, masked_pos=d["masked_pos"],
                                        return_logits=True)
        out[form + "_loss"] = np.array(loss.item())
        if c["vocab"] <= 1024:
            out[form + "_scores"] = scores.numpy()
        else:
            out[form + "_scores_cols"] = scores[:, :, SCORE_COLS].numpy()
            out[form + "_scores_lse"] = torch.logsumexp(scores.double(), -1).numpy()
            out[form + "_scores_label"] = torch.gather(scores, 2, d["masked_ids"].unsqueeze(-1)).squeeze(-1).numpy()
        norms = np.array([float(p.grad.double().norm()) if p.grad is not None else 0.0 for _, p in model.named_parameters()])
        out[form + "_grad_norms"] = norms
        for key, pname in GRAD_SAMPLE.items():
            g = dict(model.named_parameters())[pname].grad.reshape(-1)
            idx = torch.arange(64) * (g.numel() - 1) // 63
            out[form + "_grad_" + key] = g[idx].numpy()
    out["param_names"] = np.array(names)
    out["state_dict_keys"] = np.array(list(model.state_dict()))
    out["init_params"] = np.array(list(getattr(model, "init_params", [])), dtype=str)
    path = os.path.join(HERE, "%s_captioning.npz" % name)
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;", {k: float(v) for k, v in out.items() if k.endswith("_loss")})


def main():
    reference_shims.install()
    sys.modules["dataset"].build_tokenizer = bert_tokenizer      # transformers' BertTokenizer on the vocab.txt written above
    reference_shims.ensure_process_group()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(CAP_CASES)):
        run_case(name)


if __name__ == "__main__":
    main()
