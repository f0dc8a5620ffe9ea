"""XVLMForMLMCaptioning on the HIP path against the REAL reference (tests/golden/<case>_captioning.npz, make_golden_captioning.py: the
reference model on CPU fp32, same seeded weights and batches), eval mode, both collate forms, tiny and base_shallow (V = 30522, L = 58):
loss, [B, n_mask, V] prediction scores (full at tiny, a fixed column sample + per-slot log-partition at V = 30522), gradient norms and a
fixed gradient sample of the text tower, the head and the patch embedding.

Bounds (bf16 GEMM / attention operands against fp32, as test_retrieval.py / test_model_gpu.py; measured worst over the four runs in
brackets): loss 2e-3 relative [9.5e-4, tiny FG-free]; scores 1.5e-2 of max-abs [8.4e-3]; gradient norms 1.5e-2 relative [5.2e-3];
gradient samples 5e-2 of the sample's max-abs [3.1e-2]."""
import importlib

import numpy as np
import pytest
import torch

from cases import CASES
from cases_captioning import CAP_CASES, GRAD_SAMPLE, SCORE_COLS, caption_config

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLD_DIR = __import__("os").path.join(__import__("os").path.dirname(__file__), "golden")
TOL = dict(loss=2e-3, scores=1.5e-2, norm=1.5e-2, sample=5e-2)


@pytest.mark.parametrize("name", list(CAP_CASES))
@pytest.mark.parametrize("form", ["plain", "fgfree"])
def test_model_matches_reference_golden(synthetic, tmp_path, name, form):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    cc = CAP_CASES[name]
    c = CASES[cc["case"]]
    g = np.load("%s/%s_captioning.npz" % (GOLD_DIR, name))
    model = mg.XVLMForMLMCaptioning(caption_config(cc["case"], str(tmp_path)))
    synthetic.synth_state_dict(model, cc["wseed"])
    model = model.to(dev).eval()
    d = synthetic.synth_captioning_batch(cc["bseed"], cc["batch"], cc["max_tokens"], cc["max_masks"], c["image_res"], c["vocab"],
                                         fg_free=form == "fgfree")
    d = {k: v.to(dev) for k, v in d.items()}
    loss, scores = model.forward_with_scores(d["image"], d["text_ids_masked"], d["text_atts"], d["position_ids"], d["masked_pos"],
                                             d["masked_ids"], d["masked_weight"], keep_scores=True)
    loss.backward()
    errs = {}
    ref = float(g[form + "_loss"])
    errs["loss"] = abs(float(loss.detach()) - ref) / max(1.0, abs(ref))
    s = scores.detach().double().cpu()
    if form + "_scores" in g:
        want = torch.from_numpy(g[form + "_scores"]).double()
        errs["scores"] = float((s - want).abs().max() / want.abs().max())
    else:
        want = torch.from_numpy(g[form + "_scores_cols"]).double()
        errs["scores"] = max(float((s[:, :, SCORE_COLS] - want).abs().max() / want.abs().max()),
                             float((torch.logsumexp(s, -1) - torch.from_numpy(g[form + "_scores_lse"])).abs().max() / want.abs().max()))
    names = list(g["param_names"])
    params = dict(model.named_parameters())
    errs["norm"] = errs["sample"] = 0.0
    for key, pname in GRAD_SAMPLE.items():
        gr = params[pname].grad.detach().double().cpu().reshape(-1)
        norm_ref = float(g[form + "_grad_norms"][names.index(pname)])
        errs["norm"] = max(errs["norm"], abs(float(gr.norm()) - norm_ref) / norm_ref)
        idx = torch.arange(64) * (gr.numel() - 1) // 63
        ws = torch.from_numpy(g[form + "_grad_" + key]).double()
        errs["sample"] = max(errs["sample"], float((gr[idx] - ws).abs().max() / ws.abs().max()))
    print("captioning golden %s %s: %s" % (name, form, {k: "%.2e" % v for k, v in errs.items()}))
    for k, v in errs.items():
        assert v <= TOL[k], (k, v)
