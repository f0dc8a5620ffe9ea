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
from step_helpers import replays_draw_new_masks, replays_match_eager

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
    seen = replays_match_eager("grounding step", step, fwd_bwd, static, params, names, captured, data)
    assert seen[0]["loss_giou"] > 0.0 and seen[1]["loss_giou"] == 0.0 and seen[2]["loss_giou"] > 0.0
    assert all(s["loss_bbox"] > 0.0 for s in seen)


def test_replays_draw_new_dropout_masks(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model, c = _build(synthetic, train=True)
    static = _batches(synthetic, c, 1)[0]
    params = list(model.parameters())
    step = graph.GraphedStep(_step_fn(model, static, params))
    assert step.mode == "hipgraph", step.error
    replays_draw_new_masks(step, params)
