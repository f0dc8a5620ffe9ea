#!/usr/bin/env python3
"""Golden vectors for the retrieval fine-tune step: the REAL reference model's XVLMForRetrieval (models/model_retrieval.py) on CPU fp32 in eval
mode, seeded synthetic weights, the case's own batch, `idx` soft labels and injected hard negatives.  Build container only.

Recorded per case of cases_retrieval.RETRIEVAL_CASES:
  loss_itc, loss_itm                    forward(image, text_ids, text_atts, idx=idx)
  image_feat, text_feat [B, E]          the normalised ITC features of the batch
  total_grad_norm, gradnorm/<param>     float64 norms of d(loss_itc + loss_itm)
  idx, neg_idx [2, B]                   the ids and negatives used
and, in tiny_retrieval_step.npz:
  eval_min_gap                          the least distance between two ITM scores of one row of tiny_retrieval.npz's score matrices (the
                                        reference's real scores of that evaluation set, -100 fill apart): asserted > 0, i.e. no exact tie, so the
                                        declared rank rule and np.argsort agree on every ground truth inside the top k_test
  eval_<key>                            the nine figures of the declared rule on those matrices under cases_retrieval's annotation tables

Asserted: every parameter receives a gradient; no injected negative shares its row's idx; the evaluation scores hold no exact tie (were they to
tie, make_golden_retrieval.py's seeds are the ones to change).

writes tests/golden/<case>_retrieval_step.npz
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
from cases_retrieval import (EVAL_IMG2TXT, EVAL_TXT2IMG, RETRIEVAL_CASES, ranks_float64, recall_from_ranks, retrieval_batch,  # noqa: E402
                             retrieval_config)

synthetic = importlib.import_module("x2-vlm_amd.synthetic")


def recorded_eval():
    g = np.load(os.path.join(HERE, "tiny_retrieval.npz"))
    gap = np.inf
    for m in (g["score_i2t"], g["score_t2i"]):
        for row in m:
            v = np.sort(row[row != -100.0].astype(np.float64))
            assert len(v) >= 2
            gap = min(gap, float(np.diff(v).min()))
    assert gap > 0.0, "exact tie among the reference's ITM scores: change make_golden_retrieval.py's seeds"
    r_i2t = ranks_float64(g["score_i2t"], [EVAL_IMG2TXT.get(i, []) for i in range(g["score_i2t"].shape[0])])
    r_t2i = ranks_float64(g["score_t2i"], [[j] for j in EVAL_TXT2IMG])
    out = {"eval_min_gap": np.array(gap)}
    for k, v in recall_from_ranks(r_i2t, r_t2i).items():
        out["eval_" + k] = np.array(v)
    print("evaluation set: least score gap %.3e, figures %s" % (gap, {k: round(float(v), 3) for k, v in out.items() if k != "eval_min_gap"}))
    return out


def run_case(name):
    from models.model_retrieval import XVLMForRetrieval
    rc = RETRIEVAL_CASES[name]
    model = XVLMForRetrieval(config=retrieval_config(name, "/tmp/x2golden_retrieval_step_%s" % name))
    synthetic.synth_state_dict(model, rc["wseed"])
    model.eval()
    b = retrieval_batch(synthetic, name)
    ineg, tneg = b["negatives"]
    idx = b["idx"]
    for row, (i, t) in enumerate(zip(ineg, tneg)):
        assert int(idx[i]) != int(idx[row]) and int(idx[t]) != int(idx[row]), "row %d: an injected negative shares its idx" % row
    model.get_hard_negatives = lambda *a, **k: (list(ineg), list(tneg))
    feats = {}
    real = model.get_features

    def keep(image_embeds=None, text_embeds=None):
        out = real(image_embeds, text_embeds)
        if image_embeds is not None and text_embeds is not None:
            feats["image_feat"], feats["text_feat"] = (t.detach().numpy().copy() for t in out)
        return out
    model.get_features = keep
    loss_itc, loss_itm = model(b["image"], b["text_ids"], b["text_atts"], idx=idx)
    (loss_itc + loss_itm).backward()
    out = dict(loss_itc=np.array(float(loss_itc)), loss_itm=np.array(float(loss_itm)), idx=idx.numpy(), neg_idx=np.array([ineg, tneg], dtype=np.int64),
               **feats)
    total = 0.0
    for n, p in model.named_parameters():
        assert p.grad is not None, "no gradient for " + n
        v = float(p.grad.double().norm())
        out["gradnorm/" + n] = np.array(v)
        total += v * v
    out["total_grad_norm"] = np.array(total ** 0.5)
    if name == "tiny":
        out.update(recorded_eval())
    path = os.path.join(HERE, "%s_retrieval_step.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote %s (%d bytes): loss_itc %.6f loss_itm %.6f, total gradient norm %.5f" % (path, os.path.getsize(path), float(loss_itc), float(loss_itm),
                                                                                        total ** 0.5))


def main():
    reference_shims.install()
    reference_shims.ensure_process_group()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(RETRIEVAL_CASES)):
        run_case(name)


if __name__ == "__main__":
    main()
