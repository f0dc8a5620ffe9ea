"""The VQA fine-tune step (XVLMForVQA.forward(train=True)) through graph.GraphedStep: the captured step must BE the eager step.

(1) eval mode: the tiny step is captured as one hipGraph with k a DEVICE tensor and S = 8 answer rows.  Over three copy_inputs batches with
    k = [3, 1, 2] (two padding rows), [1, 1, 1] (five) and [2, 4, 2] (none) replay and eager launches from the same state agree to 1e-6 on the loss
    and 5e-3 per gradient tensor (step_helpers.replays_match_eager, the bounds of the other fine-tune steps).  Each replayed loss also equals
    the reference's formula for THAT batch's k to 1e-5, from an eager reduction='none' pass over the real rows alone with the question states
    repeated k[b] times the way the reference stacks them - no kv_idx, no padding rows - so neither the offsets nor the row -> question map
    are frozen into the graph.
(2) train mode: replays of constant inputs draw different dropout masks and stay finite."""
import importlib
import tempfile
from types import SimpleNamespace

import pytest
import torch

from cases_vqa_train import VQA_TRAIN_CASES, vqa_train_batch, vqa_train_config
from step_helpers import replays_draw_new_masks, replays_match_eager

pytestmark = pytest.mark.gpu
dev = "cuda"
S = 8
KS = ([3, 1, 2], [1, 1, 1], [2, 4, 2])


def _build(synthetic, train):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    model = mg.XVLMForVQA(vqa_train_config("tiny", tempfile.mkdtemp()))
    synthetic.synth_state_dict(model, VQA_TRAIN_CASES["tiny"]["wseed"])
    return model.to(dev).train(train)


def _batches(synthetic, ks):
    out = []
    for i, k in enumerate(ks):
        b = vqa_train_batch(synthetic, "tiny", k=k, bseed=VQA_TRAIN_CASES["tiny"]["bseed"] + i)
        n, La = b["answer_ids"].shape
        ids, atts, weights = torch.zeros(S, La, dtype=torch.int64), torch.zeros(S, La, dtype=torch.int64), torch.zeros(S)
        ids[:n], atts[:n], weights[:n] = b["answer_ids"], b["answer_atts"], b["weights"]       # the rows behind sum(k): id 0, attention 0
        out.append(dict(image=b["image"].to(dev), question_ids=b["question_ids"].to(dev), question_atts=b["question_atts"].to(dev),
                        answer_ids=ids.to(dev), answer_atts=atts.to(dev), weights=weights.to(dev), k=b["k"].to(dev)))
    return out


def _spaces(static):
    return (SimpleNamespace(input_ids=static["question_ids"], attention_mask=static["question_atts"]),
            SimpleNamespace(input_ids=static["answer_ids"], attention_mask=static["answer_atts"]))


def _step_fn(model, static, params):
    q, a = _spaces(static)

    def fwd_bwd():
        for p in params:
            p.grad = None
        loss = model(static["image"], q, a, k=static["k"], weights=static["weights"], train=True)
        loss.backward()
        return dict(loss=loss.detach())
    return fwd_bwd


def test_graph_replay_is_the_eager_step(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model = _build(synthetic, train=False)
    data = _batches(synthetic, KS)
    static = {k: v.clone() for k, v in data[0].items()}
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    fwd_bwd = _step_fn(model, static, params)
    step = graph.GraphedStep(fwd_bwd)
    assert step.mode == "hipgraph", step.error
    captured = [p.grad for p in params]                      # the arenas the graph writes on every replay
    assert all(g is not None for g in captured)

    def reference_loss(i, b):
        # This forward comes first: the weight bank re-casts at the first forward after a backward, and the update writes through p.data
        n, B = sum(KS[i]), len(KS[i])
        with torch.no_grad():
            image_embeds, image_atts = model.get_vision_embeds(static["image"])
            states = model.text_encoder(static["question_ids"], attention_mask=static["question_atts"], encoder_hidden_states=image_embeds,
                                        encoder_attention_mask=image_atts, return_dict=True).last_hidden_state
            rows = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(KS[i], device=dev))
            ids = static["answer_ids"][:n]
            per_answer = model.text_decoder(ids, attention_mask=static["answer_atts"][:n], encoder_hidden_states=states[rows].contiguous(),
                                            encoder_attention_mask=static["question_atts"][rows], labels=ids.masked_fill(ids == 0, -100),
                                            reduction="none").loss
        want = float((static["weights"][:n].double() * per_answer.double()).sum() / B)

        def check(lg):
            print("vqa train step, batch %d: k = %s, reference loss %.6f" % (i, KS[i], want))
            assert abs(lg["loss"] - want) <= 1e-5 * want, (i, lg["loss"], want)
        return check

    seen = replays_match_eager("vqa train step", step, fwd_bwd, static, params, names, captured, data, before=reference_loss)
    assert all(s["loss"] > 0.0 for s in seen) and len(set(s["loss"] for s in seen)) == 3


def test_replays_draw_new_dropout_masks(synthetic):
    graph = importlib.import_module("x2-vlm_amd.graph")
    model = _build(synthetic, train=True)
    assert model.text_decoder.config.hidden_dropout_prob > 0
    static = _batches(synthetic, KS[:1])[0]
    params = list(model.parameters())
    step = graph.GraphedStep(_step_fn(model, static, params))
    assert step.mode == "hipgraph", step.error
    replays_draw_new_masks(step, params)
