#!/usr/bin/env python3
"""Golden vectors for the VQA training step: the REAL reference model's XVLMForVQA.forward(train=True) (models/model_generation.py:517-550)
and its backward on CPU fp32, eval mode, seeded synthetic weights, the case's seeded training batch (synthetic.synth_vqa_train_batch).
Build container only.

Recorded per case (a forward hook on text_decoder gives the per-answer losses, as make_golden_vqa.py records the candidate pass):
  loss []                     what forward returned
  answer_loss [S]             the decoder's reduction='none' loss, one value per answer row
  k [B], weights [S]          the batch's answers per question and answer weights
  total_grad_norm []          float64 norm over all parameters
  gradnorm/<param> []         float64 norm per parameter
  word_sample [64]            the gradient of text_decoder.bert.embeddings.word_embeddings.weight at cases_vqa_train.word_sample_index:
                              rows of tokens that occur in the answers (lookup and tied head both contribute there)

Asserted, so a seed that breaks one fails the run: every parameter receives a gradient; loss == sum(weights * answer_loss) / B to 1e-6 in
float64.

writes tests/golden/<case>_vqa_train.npz for VQA_TRAIN_CASES
"""
import importlib
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import reference_shims  # noqa: E402
from cases_vqa_train import VQA_TRAIN_CASES, WORD, vqa_train_batch, vqa_train_config, word_sample_index  # noqa: E402

synthetic = importlib.import_module("x2-vlm_amd.synthetic")


def run_case(name):
    from models.model_generation import XVLMForVQA
    tc = VQA_TRAIN_CASES[name]
    model = XVLMForVQA(config=vqa_train_config(name, tempfile.mkdtemp(prefix="x2golden_vqa_train_")))
    synthetic.synth_state_dict(model, tc["wseed"])
    model.eval()
    b = vqa_train_batch(synthetic, name)
    B, S = b["image"].shape[0], b["answer_ids"].shape[0]
    dec_out = []
    hook = model.text_decoder.register_forward_hook(lambda m, i, o: dec_out.append(o))
    try:
        loss = model(b["image"], SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"]),
                     SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"]), k=b["k"].tolist(), weights=b["weights"],
                     train=True)
    finally:
        hook.remove()
    loss.backward()
    assert len(dec_out) == 1
    answer_loss = dec_out[0].loss.detach()
    assert answer_loss.shape == (S,)
    want = float((b["weights"].double() * answer_loss.double()).sum() / B)
    assert abs(float(loss.detach().double()) - want) <= 1e-6 * abs(want), (float(loss), want)
    out = dict(loss=np.array(loss.detach().item()),answer_loss=answer_loss.numpy(), k=b["k"].numpy(), weights=b["weights"].numpy())
    total = 0.0
    params = dict(model.named_parameters())
    for n, p in params.items():
        assert p.grad is not None, "no gradient for " + n
        sq = float(p.grad.double().pow(2).sum())
        total += sq
        out["gradnorm/" + n] = np.array(sq ** 0.5)
    out["total_grad_norm"] = np.array(total ** 0.5)
    gw = params[WORD].grad
    out["word_sample"] = gw.reshape(-1)[torch.tensor(word_sample_index(b["answer_ids"], gw.shape[1]))].numpy()
    path = os.path.join(HERE, "%s_vqa_train.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    tiny = sorted((float(v), n[len("gradnorm/"):]) for n, v in out.items() if n.startswith("gradnorm/"))[:4]
    print("wrote %s, %d bytes: loss %.6f, answer losses %s, %d parameters with a gradient, total norm %.5f; smallest norms %s"
          % (path, os.path.getsize(path), float(out["loss"]), np.round(answer_loss.numpy(), 4), len(params), total ** 0.5, tiny))


def main():
    reference_shims.install()
    reference_shims.ensure_process_group()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(VQA_TRAIN_CASES)):
        run_case(name)


if __name__ == "__main__":
    main()
