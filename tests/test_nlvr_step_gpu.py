"""The NLVR2 fine-tune step through graph.GraphedStep: the captured step must BE the eager step.

(1) eval mode: the tiny step is captured as one hipGraph; over three copy_inputs batches - the second has an ignored target, so n_valid changes
    on the device between replays - replay and eager launches from the same state agree to 1e-6 on the loss and 5e-3 per gradient tensor (the
    bounds of tests/test_grounding_step_gpu.py and tests/test_graph_gpu.py::test_graph_replay_is_the_eager_step).
(2) train mode (the 2B-row text pass): replays of constant inputs draw different dropout masks and stay finite."""
import importlib
import tempfile

import pytest
import torch

from cases import CASES
from cases_nlvr import NLVR_CASES, nlvr_batch, nlvr_config

pytestmark = pytest.mark.gpu
dev = "cuda"


def _build(synthetic, train):
    mcl = importlib.import_module("x2-vlm_amd.model_classification")
    model = mcl.XVLMForNLVR(nlvr_config("tiny", tempfile.mkdtemp()))
    synthetic.synth_state_dict(model, NLVR_CASES["tiny"]["wseed"])
    return model.to(dev).train(train), CASES["tiny"]


def _batches(synthetic, c, n, ignore=()):
    out = []
    for i in range(n):
        b = nlvr_batch(synthetic, "tiny", bseed=c["bseed"] + i, ragged=False)
        if i in ignore:
            b["targets"][b["targets"].numel() - 1] = -100
        out.append({k: v.to(dev) for k, v in b.items()})
    return out


def _step_fn(model, static, params):
    def fwd_bwd():
        for p in params:
            p.grad = None
        loss = model(static["image"], static["text_ids"], static["text_atts"], static["targets"], train=True)
        loss.backward()
        return dict(loss=loss.detach())
    return fwd_bwd


def test_graph_replay_is_the_eager_step(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model, c = _build(synthetic, train=False)
    data = _batches(synthetic, c, 3, ignore=(1,))
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
        print("nlvr step, batch %d: eager %s, replay %s, worst gradient tensor difference %.2e" % (i, le, lg, worst))
        seen.append(lg)
        with torch.no_grad():                                # the next state, through p.data as transformers' AdamW moves it
            for p, g in zip(params, eager):
                p.data.add_(g, alpha=-0.02)
    assert all(s["loss"] > 0.0 for s in seen) and len(set(s["loss"] for s in seen)) == 3


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
