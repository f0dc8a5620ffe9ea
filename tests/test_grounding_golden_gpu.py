"""XVLMForGrounding on the HIP path against the REAL reference's run (tests/golden/<case>_grounding.npz, make_golden_grounding.py: CPU fp32,
eval mode, same seeded weights, batch and target boxes): tiny, large_shallow (384 px, N = 577, width 1024) and tiny with one target box of
negative width.

Bounds.  Coordinates: 5e-3 of the golden's max-abs, POINTWISE["bbox_coord"] of tests/test_model_gpu.py.  loss_bbox: absolute, at most
4 x 5e-3 (L1 is 1-Lipschitz per coordinate, four coordinates per row, mean over rows).  loss_giou: relative.  Gradient norms, normalised as
tests/test_model_gpu.py does: per tensor |norm - golden| / max(golden, 1e-2 x the golden total), and the total's relative error - both for
d(loss_bbox + loss_giou) and, against its own golden, for d(loss_bbox) alone, so a missing GIoU gradient cannot hide in the sum.  The path is
deterministic (no atomics), so each bound is about 1.5 x the value measured on the MI355X, rounded up; the margin is for later harmless
reorderings.  The generator keeps every max / min / abs / clamp argument 2e-2 from its kink, four coordinate bounds, so bf16 operand error
cannot flip a sub-gradient.

Measured on the MI355X (printed by the tests; tiny / large_shallow / tiny_degenerate):
  coordinates, of max-abs            2.58e-3 / 1.83e-3 / 2.58e-3      (bound 5e-3)
  |loss_bbox - reference|            3.86e-4 / 5.10e-4 / 5.44e-4      (bound 9e-4)
  loss_giou, relative                1.18e-3 / 4.19e-4 / exactly 0    (bound 2e-3)
  d(bbox + giou): worst tensor norm  8.10e-3 / 2.86e-3 / 3.22e-3      (bound 1.3e-2);  total norm 7.51e-4 / 1.40e-3 / 2.56e-4  (bound 2.2e-3)
  d(bbox alone):  worst tensor norm  5.40e-3 / 1.17e-3 / 3.22e-3      (bound 1.3e-2);  total norm 2.35e-5 / 1.28e-4 / 2.56e-4  (bound 2.2e-3)
  inference against the training call's coordinates: within 1e-6; evaluation: the golden's 96 hits and all four accuracies."""
import importlib
import os

import numpy as np
import pytest
import torch

from cases_grounding import GROUNDING_CASES, SPLITS, eval_set, grounding_batch, grounding_config

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
COORD = 5e-3
# about 1.5 x the worst measured value (docstring), rounded up
BOUND = dict(loss_bbox=9e-4, loss_giou=2e-3, gradnorm=1.3e-2, total=2.2e-3)
assert BOUND["loss_bbox"] <= 4 * COORD


def norms_of(model):
    out = {}
    for n, p in model.named_parameters():
        assert p.grad is not None, "no gradient for " + n
        assert bool(torch.isfinite(p.grad).all()), n
        out[n] = float(p.grad.double().norm())
    return out


@pytest.fixture(scope="module", params=list(GROUNDING_CASES))
def run(request, synthetic, tmp_path_factory):
    """Model, golden and the runs every test reads (computed once per case and left unchanged)."""
    name = request.param
    mgr = importlib.import_module("x2-vlm_amd.model_grounding")
    model = mgr.XVLMForGrounding(grounding_config(name, str(tmp_path_factory.mktemp(name))))
    synthetic.synth_state_dict(model, GROUNDING_CASES[name]["wseed"])
    model = model.to(dev).eval()
    b = {k: v.to(dev) for k, v in grounding_batch(synthetic, name).items()}
    coord, lb, lg = model(b["image"], b["text_ids"], b["text_atts"], b["target_bbox"])
    (lb + lg).backward()
    both = norms_of(model)
    model.zero_grad(set_to_none=True)
    _, lb2, _ = model(b["image"], b["text_ids"], b["text_atts"], b["target_bbox"])
    lb2.backward()
    bbox_only = norms_of(model)
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        infer = model(b["image"], b["text_ids"], b["text_atts"])
    torch.cuda.synchronize()
    return dict(name=name, g=np.load("%s/%s_grounding.npz" % (GOLD_DIR, name)), coord=coord.detach().cpu(), loss_bbox=float(lb.detach()), loss_giou=float(lg.detach()),
                loss_bbox2=float(lb2.detach()), both=both, bbox_only=bbox_only, infer=infer.cpu(), degenerate=bool(GROUNDING_CASES[name].get("degenerate")))


def test_coordinates_and_losses_match_the_reference(run):
    g = run["g"]
    ref = g["output_coord"]
    e_c = float(np.abs(run["coord"].numpy() - ref).max()) / float(np.abs(ref).max())
    e_b = abs(run["loss_bbox"] - float(g["loss_bbox"]))
    ref_g = float(g["loss_giou"])
    e_g = abs(run["loss_giou"] - ref_g) / ref_g if ref_g else abs(run["loss_giou"])
    print("grounding %s: coord %.3e of max-abs (bound %.0e); |loss_bbox - ref| %.3e (bound %.1e); loss_giou rel %.3e (bound %.1e)"
          % (run["name"], e_c, COORD, e_b, BOUND["loss_bbox"], e_g, BOUND["loss_giou"]))
    assert run["coord"].shape == ref.shape and run["coord"].dtype == torch.float32
    assert e_c <= COORD and e_b <= BOUND["loss_bbox"]
    assert run["loss_bbox2"] == run["loss_bbox"]
    if run["degenerate"]:
        assert run["loss_giou"] == 0.0 and ref_g == 0.0                      # exactly: the early-out, decided on the device
    else:
        assert e_g <= BOUND["loss_giou"]


def grad_report(run, got, prefix, total_key):
    g = run["g"]
    total = float(g[total_key])
    worst, worst_name = 0.0, ""
    for n, v in got.items():
        ref = float(g[prefix + n])
        e = abs(v - ref) / max(ref, 1e-2 * total)
        if e > worst:
            worst, worst_name = e, n
    e_t = abs(sum(v * v for v in got.values()) ** 0.5 - total) / total
    return worst, worst_name, e_t


def test_gradient_norms_match_the_reference(run):
    """d(loss_bbox + loss_giou) and d(loss_bbox) alone, each against its own golden; in the degenerate case the two are the same gradient"""
    for got, prefix, total_key, what in ((run["both"], "gradnorm/", "total_grad_norm", "bbox + giou"),
                                         (run["bbox_only"], "gradnorm_bbox/", "total_grad_norm_bbox", "bbox alone")):
        worst, worst_name, e_t = grad_report(run, got, prefix, total_key)
        print("grounding %s, d(%s): worst per-tensor norm error %.3e (%s; bound %.1e), total norm %.3e (bound %.1e)"
              % (run["name"], what, worst, worst_name, BOUND["gradnorm"], e_t, BOUND["total"]))
        assert worst <= BOUND["gradnorm"] and e_t <= BOUND["total"]
    if run["degenerate"]:
        assert run["both"] == run["bbox_only"]                               # the GIoU term contributes no gradient at all: the same bits
        worst, _, e_t = grad_report(run, run["both"], "gradnorm_bbox/", "total_grad_norm_bbox")
        assert worst <= BOUND["gradnorm"] and e_t <= BOUND["total"]
    else:
        assert run["both"] != run["bbox_only"]


def test_inference_equals_the_training_coordinates(run):
    assert float((run["infer"] - run["coord"]).abs().max()) <= 1e-6


def test_grounding_eval_bbox_reproduces_the_reference(synthetic):
    mgr = importlib.import_module("x2-vlm_amd.model_grounding")
    g = np.load("%s/tiny_grounding.npz" % GOLD_DIR)
    pred, ref_box, size, split = eval_set()
    iou, hit = mgr.grounding_iou(torch.from_numpy(pred).to(dev), ref_box, size)
    assert hit.dtype == torch.bool and float(np.abs(iou.cpu().numpy() - g["eval_iou"]).max()) <= 1e-5
    assert np.array_equal(hit.cpu().numpy(), g["eval_hit"])
    res = mgr.grounding_eval_bbox(torch.from_numpy(pred).to(dev), torch.from_numpy(ref_box), torch.from_numpy(size).to(dev), split)
    assert sorted(res) == sorted(s + "_d" for s in SPLITS)
    for k, v in res.items():
        assert v == float(g["eval_acc/" + k]), k
    res = mgr.grounding_eval_bbox(torch.from_numpy(pred).to(dev), ref_box, size)
    assert list(res) == ["score"] and res["score"] == float(g["eval_acc/score"])
