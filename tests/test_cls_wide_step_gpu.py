"""The VQA classification fine-tune step (XVLMForVQAClassification) through graph.GraphedStep: the captured step must BE the eager step.

The tiny model in train mode (self.training, every dropout and DropPath rate at zero so that two launches of one state can be compared) is captured
as one hipGraph.  k is a DEVICE tensor: the entry offsets are its prefix sum computed on the device, so nothing about the answers per row is frozen
into the graph; T is fixed at 8 and the tail behind sum(k) is padded with -100 targets of weight 0.  Over three copy_inputs batches - the second has
a row without answers, the third uses half of the T slots - replay and eager launches from the same state agree to 1e-6 on the loss and 5e-3 per
gradient tensor (the bounds of tests/test_nlvr_step_gpu.py and tests/test_graph_gpu.py::test_graph_replay_is_the_eager_step)."""
import importlib
import tempfile

import pytest
import torch

from cases import CASES
from cases_cls import CLS_CASES, cls_batch, cls_config
from step_helpers import replays_match_eager

pytestmark = pytest.mark.gpu
dev = "cuda"
T = 8
KS = ([2, 1, 3, 1], [3, 0, 2, 2], [1, 1, 1, 1])


def _build(synthetic):
    mcl = importlib.import_module("x2-vlm_amd.model_classification")
    cfg = dict(cls_config("tiny_vqacls", tempfile.mkdtemp()), drop_path_rate=0.0, dropout=0.0)
    model = mcl.XVLMForVQAClassification(cfg)
    model.text_encoder.config.attention_probs_dropout_prob = 0.0
    synthetic.synth_state_dict(model, CLS_CASES["tiny_vqacls"]["wseed"])
    return model.to(dev).train(), CASES["tiny"]


def _batches(synthetic, c):
    out = []
    C = CLS_CASES["tiny_vqacls"]["labels"]
    for i, k in enumerate(KS):
        b = cls_batch(synthetic, "tiny_vqacls", bseed=c["bseed"] + i, ragged=False)
        g = torch.Generator().manual_seed(100 + i)
        n = sum(k)
        targets = torch.full((T,), -100, dtype=torch.int64)
        targets[:n] = torch.randint(0, C, (n,), generator=g)
        weights = torch.zeros(T)
        weights[:n] = torch.randint(1, 11, (n,), generator=g).float() / 10.0
        out.append(dict(image=b["image"].to(dev), text_ids=b["text_ids"].to(dev), text_atts=b["text_atts"].to(dev), targets=targets.to(dev),
                        weights=weights.to(dev), k=torch.tensor(k, dtype=torch.int64, device=dev)))
    return out


def _step_fn(model, static, params):
    def fwd_bwd():
        for p in params:
            p.grad = None
        loss = model(static["image"], static["text_ids"], static["text_atts"], targets=static["targets"], k=static["k"], weights=static["weights"],
                     train=True)
        loss.backward()
        return dict(loss=loss.detach())
    return fwd_bwd


def test_graph_replay_is_the_eager_step(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model, c = _build(synthetic)
    assert model.training
    data = _batches(synthetic, c)
    static = {k: v.clone() for k, v in data[0].items()}
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    fwd_bwd = _step_fn(model, static, params)
    step = graph.GraphedStep(fwd_bwd)
    assert step.mode == "hipgraph", step.error
    captured = [p.grad for p in params]                      # the arenas the graph writes on every replay
    assert all(g is not None for g in captured)

    def reference_loss(i, b):
        # the reference's formula for THIS batch's k on the logits of the same state (the graph must not have frozen the first batch's offsets).
        # This forward comes first: the weight bank re-casts at the first forward after a backward, and the update below writes through p.data
        with torch.no_grad():
            prediction = model(static["image"], static["text_ids"], static["text_atts"], train=False).double().cpu()
        rows = torch.repeat_interleave(torch.arange(4), torch.tensor(KS[i]))
        n = sum(KS[i])
        nll = torch.nn.functional.cross_entropy(prediction[rows], b["targets"][:n].cpu(), reduction="none")
        want = float((b["weights"][:n].cpu().double() * nll).sum() / 4)

        def check(lg):
            print("vqa-cls step, batch %d: k = %s, reference loss %.6f" % (i, KS[i], want))
            assert abs(lg["loss"] - want) <= 1e-5 * want, (i, lg["loss"], want)
        return check

    seen = replays_match_eager("vqa-cls step", step, fwd_bwd, static, params, names, captured, data, before=reference_loss)
    assert all(s["loss"] > 0.0 for s in seen) and len(set(s["loss"] for s in seen)) == 3
