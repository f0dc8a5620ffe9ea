"""XVLMForMLMCaptioning on the HIP path (tiny geometry, both collate forms): the loss equals the float64 label-smoothed, weight-normalised
loss of the model's own prediction scores; explicit position ids are honoured (a shifted id list equals a shifted position table); the
[B, L, L] mask reaches every layer (tril: no output depends on a later token, fusion layers included); a train-mode step is bit-reproducible.

Tolerance: the loss against float64 of the scores 2e-6 relative [measured worst 9.6e-8]: the fused loss recomputes the same bf16-operand
logits inside the decoder GEMM and forms the KL in fp32.  The model against the reference itself: test_captioning_golden_gpu.py."""
import importlib

import pytest
import torch

from cases import CASES, model_config

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
WSEED = 41


def caption_config(tmp_path):
    cfg = model_config("tiny", str(tmp_path))
    cfg.update(label_smoothing=0.1, prompt="", cls_token_id=1)
    return cfg


def build(synthetic, tmp_path):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    model = mg.XVLMForMLMCaptioning(caption_config(tmp_path))
    synthetic.synth_state_dict(model, WSEED)
    return model.to(dev)


def batch(synthetic, fg_free, seed=5):
    c = CASES["tiny"]
    d = synthetic.synth_captioning_batch(seed, 3, 12, 4, c["image_res"], c["vocab"], fg_free=fg_free)
    return {k: v.to(dev) for k, v in d.items()}


def ref_loss(scores, labels, w, V, ignore, ls):
    z = scores.double().reshape(-1, V)
    labels, w = labels.reshape(-1).cpu(), w.reshape(-1).double().cpu()
    q = torch.full(z.shape, ls / (V - 2), dtype=torch.float64)
    q[:, ignore] = 0
    q.scatter_(1, labels.view(-1, 1), 1.0 - ls)
    q[labels == ignore] = 0
    kl = torch.nn.functional.kl_div(torch.log_softmax(z.cpu(), -1), q, reduction="none").sum(-1)
    return float((kl * w / (w.sum() + 1e-5)).sum())


@pytest.mark.parametrize("fg_free", [False, True])
def test_loss_matches_float64_of_scores(synthetic, tmp_path, fg_free):
    model = build(synthetic, tmp_path).eval()
    d = batch(synthetic, fg_free)
    args = (d["image"], d["text_ids_masked"], d["text_atts"], d["position_ids"], d["masked_pos"], d["masked_ids"], d["masked_weight"])
    with torch.no_grad():
        loss, scores = model.forward_with_scores(*args, keep_scores=True)
        loss2 = model(*args)
    assert scores.shape == (3, 4, 512)
    want = ref_loss(scores, d["masked_ids"], d["masked_weight"], 512, 1, 0.1)
    err = abs(float(loss) - want) / max(1.0, abs(want))
    print("captioning loss fg_free=%s: %.6f vs %.6f (rel %.2e)" % (fg_free, float(loss), want, err))
    assert err < 2e-6 and float(loss) == float(loss2)
    # gradients flow into every trained tensor of the text side, finite
    model.train()
    for p in model.parameters():
        p.grad = None
    model(*args).backward()
    te = model.text_encoder
    for t in (te.bert.embeddings.position_embeddings.weight, te.bert.embeddings.word_embeddings.weight,
              te.bert.encoder.layer[0].attention.self.query.weight, te.cls.predictions.bias):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0


def test_position_ids_are_honoured(synthetic, tmp_path):
    model = build(synthetic, tmp_path).eval()
    d = batch(synthetic, True)
    te = model.text_encoder
    ids, atts = d["text_ids_masked"], d["text_atts"][:, :, :]
    L = ids.shape[1]
    with torch.no_grad():
        plain = te.bert(ids, attention_mask=atts, mode="text").last_hidden_state
        same = te.bert(ids, attention_mask=atts, mode="text", position_ids=torch.arange(L, device=dev).unsqueeze(0)).last_hidden_state
        assert torch.equal(plain, same)
        shifted = te.bert(ids, attention_mask=atts, mode="text", position_ids=torch.arange(L, device=dev).unsqueeze(0) + 3).last_hidden_state
        assert not torch.equal(plain, shifted)
        pos = te.bert.embeddings.position_embeddings.weight
        keep = pos.detach().clone()
        pos.data[:L] = keep[3:L + 3]
        moved = te.bert(ids, attention_mask=atts, mode="text").last_hidden_state
        pos.data.copy_(keep)
        assert torch.equal(shifted, moved)
        # BertForMaskedLM.forward passes them on (it used to drop them)
        a = te(ids, attention_mask=atts, masked_pos=d["masked_pos"], return_logits=True, mode="text")
        b = te(ids, attention_mask=atts, masked_pos=d["masked_pos"], return_logits=True, mode="text", position_ids=d["position_ids"])
        assert not torch.equal(a, b)


def test_tril_mask_reaches_every_layer(synthetic, tmp_path):
    model = build(synthetic, tmp_path).eval()
    d = batch(synthetic, False)
    ids, atts = d["text_ids_masked"].clone(), d["text_atts"]
    with torch.no_grad():
        img, img_atts = model.get_vision_embeds(d["image"])
        h1 = model.text_encoder.bert(ids, attention_mask=atts, encoder_hidden_states=img, encoder_attention_mask=img_atts).last_hidden_state
        ids[:, 7:] = 9
        h2 = model.text_encoder.bert(ids, attention_mask=atts, encoder_hidden_states=img, encoder_attention_mask=img_atts).last_hidden_state
    assert torch.equal(h1[:, :7], h2[:, :7]) and not torch.equal(h1[:, 7:], h2[:, 7:])


def test_train_step_is_bit_reproducible(synthetic, tmp_path):
    xbert = importlib.import_module("x2-vlm_amd.xbert")
    outs = []
    for _ in range(2):
        model = build(synthetic, tmp_path).train()
        d = batch(synthetic, True)
        xbert._FIXED_SEEDS[:] = [111, 222, 333, 444, 555, 666]
        loss = model(d["image"], d["text_ids_masked"], d["text_atts"], d["position_ids"], d["masked_pos"], d["masked_ids"], d["masked_weight"])
        loss.backward()
        outs.append([loss.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None])
    xbert._FIXED_SEEDS[:] = []
    assert len(outs[0]) == len(outs[1]) and len(outs[0]) > 10
    for a, b in zip(*outs):
        assert torch.equal(a, b)
