"""The grounding fine-tune step through graph.GraphedStep: the captured step must BE the eager step, the degenerate-box flag included.

(1) eval mode: the tiny step is captured as one hipGraph; over three copy_inputs batches - the second has a target box of negative width -
    replay and eager launches from the same state agree to 1e-6 on the losses and 5e-3 per gradient tensor (the bounds of
    tests/test_graph_gpu.py::test_graph_replay_is_the_eager_step).  The captured launch sequence is the same for all three: loss_giou is
    exactly 0 in the second replay and positive in the others only because the early-out is decided on the device.
(2) train mode: replays of constant inputs draw different dropout masks and stay finite."""
import importlib
import tempfile

import pytest
import torch

from cases import CASES
from cases_grounding import GROUNDING_CASES, grounding_config, target_boxes

pytestmark = pytest.mark.gpu
dev = "cuda"


def _build(synthetic, train):
    mgr = importlib.import_module("x2-vlm_amd.model_grounding")
    model = mgr.XVLMForGrounding(grounding_config("tiny", tempfile.mkdtemp()))
    synthetic.synth_state_dict(model, GROUNDING_CASES["tiny"]["wseed"])
    return model.to(dev).train(train), CASES["tiny"]


def _batches(synthetic, c, n, degenerate=()):
    out = []
    for i in range(n):
        b = synthetic.synth_batch(c["bseed"] + i, c["batch"], c["seq_len"], c["image_res"], c["vocab"], c["max_masks"], ragged=False)
        t = target_boxes(GROUNDING_CASES["tiny"]["tseed"] + i, c["batch"])
        if i in degenerate:
            t[c["batch"] - 1, 2] = -0.25
        out.append(dict(image=b["image"].to(dev), text_ids=b["text_ids"].to(dev), text_atts=b["text_atts"].to(dev),
                        target_bbox=torch.from_numpy(t).to(dev)))
    return out


def _step_fn(model, static, params):
    def fwd_bwd():
        for p in params:
            p.grad = None
        coord, loss_bbox, loss_giou = model(static["image"], static["text_ids"], static["text_atts"], static["target_bbox"])
        (loss_bbox + loss_giou).backward()
        return dict(loss_bbox=loss_bbox.detach(), loss_giou=loss_giou.detach())
    return fwd_bwd


def test_graph_replay_is_the_eager_step(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model, c = _build(synthetic, train=False)
    data = _batches(synthetic, c, 3, degenerate=(1,))
    static = {k: v.clone() for k, v in data[0].items()}
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    fwd_bwd = _step_fn(model, static, params)
    step = graph.GraphedStep(fwd_bwd)
    assert step.mode == "hipgraph", step.error
    captured = [p.grad for p in params]                      # the arenas the graph writes on every replay
    assert all(g is not None for g in captured)
    seen = []
    for i, b in enumerate(data):
        graph.GraphedStep.copy_inputs(static, b)
        le = {k: float(v) for k, v in fwd_bwd().items()}     # eager launches (re-binds .grad to fresh tensors)
        torch.cuda.synchronize()
        eager = [p.grad.detach().clone() for p in params]
        lg = {k: float(v) for k, v in step().items()}        # the same state through the captured graph
        torch.cuda.synchronize()
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-6 * max(1.0, abs(le[k])), (i, k, le[k], lg[k])
        total = sum(float(g.double().pow(2).sum()) for g in eager) ** 0.5
        worst = 0.0
        for n, ge, gg in zip(names, eager, captured):
            assert bool(torch.isfinite(gg).all()), n
            if "key.bias" not in n:                          # key biases: analytically zero gradient, pure rounding noise
                err = float((ge.double() - gg.double()).norm()) / max(float(ge.double().norm()), 1e-2 * total)
                worst = max(worst, err)
                assert err <= 5e-3, (i, n, err)
        print("grounding step, batch %d: eager %s, replay %s, worst gradient tensor difference %.2e" % (i, le, lg, worst))
        seen.append(lg)
        with torch.no_grad():                                # the next state, through p.data as transformers' AdamW moves it
            for p, g in zip(params, eager):
                p.data.add_(g, alpha=-0.02)
    assert seen[0]["loss_giou"] > 0.0 and seen[1]["loss_giou"] == 0.0 and seen[2]["loss_giou"] > 0.0
    assert all(s["loss_bbox"] > 0.0 for s in seen)


def test_replays_draw_new_dropout_masks(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model, c = _build(synthetic, train=True)
    static = _batches(synthetic, c, 1)[0]
    params = list(model.parameters())
    step = graph.GraphedStep(_step_fn(model, static, params))
    assert step.mode == "hipgraph", step.error
    seen = []
    for _ in range(4):
        loss = step()
        seen.append(tuple(round(float(v), 6) for v in loss.values()))
        assert all(bool(torch.isfinite(p.grad).all()) for p in params)
    assert all(all(x == x and abs(x) < 1e4 for x in s) for s in seen)   # finite
    assert len(set(seen)) == 4, seen                                    # same inputs, four different masks
