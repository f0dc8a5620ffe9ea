"""Captioning fine-tune, host side (no GPU): the mirror's public surface (XVLMForMLMCaptioning, position_ids / 3-D masks reaching
BertModel, unsupported keywords refused), the seeded captioning collate in both forms, and a float64 restatement of the label-smoothed
loss in the chunk-statistics form the fused kernels evaluate, pinned to LabelSmoothingLoss's definition."""
import importlib
import inspect
import os

import numpy as np

import pytest
import torch

from cases import model_config


def caption_config(tmp_path, case="tiny"):
    cfg = model_config(case, str(tmp_path))
    cfg.update(label_smoothing=0.1, prompt="a picture of ", cls_token_id=1 if case.startswith("tiny") else 101)
    return cfg


def test_model_surface(tmp_path):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    model = mg.XVLMForMLMCaptioning(caption_config(tmp_path))
    sig = inspect.signature(model.forward)
    assert list(sig.parameters) == ["image", "input_ids_masked", "attention_mask", "position_ids", "masked_pos", "masked_ids", "masked_weight"]
    assert list(inspect.signature(model.load_pretrained).parameters) == ["ckpt_rpath", "config", "is_eval"]
    # parameter names, state-dict keys and init_params of the REAL reference model (recorded by make_golden_captioning.py)
    for case in ("tiny", "base_shallow"):
        g = np.load(os.path.join(os.path.dirname(__file__), "golden", "%s_captioning.npz" % case))
        m = model if case == "tiny" else mg.XVLMForMLMCaptioning(caption_config(tmp_path / case, case))
        assert [n for n, _ in m.named_parameters()] == list(g["param_names"])
        # (the reference's state dict also lists the MLM head's bias a second time, under the tied decoder's name - the text
        # encoder mirror, shared with pre-training, keeps one entry)
        skip = ("relative_position_index", "cls.predictions.decoder.bias")
        assert sorted(k for k in m.state_dict() if not k.endswith(skip)) == sorted(k for k in g["state_dict_keys"] if not k.endswith(skip))
        assert sorted(m.init_params) == sorted(g["init_params"])
    assert model.label_smoothing == 0.1 and model.ignore_index == 1 and model.tgt_vocab_size == 512
    with pytest.raises(NotImplementedError, match="follow-up"):
        model.generate(None)


def test_text_encoder_keywords(tmp_path):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    model = mg.XVLMForMLMCaptioning(caption_config(tmp_path))
    te = model.text_encoder
    assert "position_ids" in inspect.signature(te.forward).parameters
    assert "position_ids" in inspect.signature(te.bert.forward).parameters
    assert "position_ids" in inspect.signature(te.bert.embeddings.forward).parameters
    ids = torch.zeros(1, 4, dtype=torch.long)
    for call in (lambda: te(ids, masked_pos=torch.zeros(1, 1, dtype=torch.long), head_mask=torch.ones(1)),
                 lambda: te.bert(ids, head_mask=torch.ones(1))):
        with pytest.raises(NotImplementedError, match="head_mask"):
            call()


@pytest.mark.parametrize("fg_free", [False, True])
def test_synthetic_captioning_batch_rules(synthetic, fg_free):
    B, T, M = 4, 40, 18
    d = synthetic.synth_captioning_batch(7, B, T, M, 32, 30522, fg_free=fg_free)
    L = T + M if fg_free else T
    assert d["text_atts"].shape == (B, L, L) and d["position_ids"].shape == (B, L) and d["masked_weight"].shape == (B, M)
    tri = torch.tril(torch.ones(L, L, dtype=torch.long))
    for b in range(B):
        k = int(d["masked_weight"][b].sum())
        assert k >= 1 and bool((d["masked_ids"][b, k:] == 101).all()) and bool((d["masked_pos"][b, k:] == 0).all())
        slots = d["masked_pos"][b, :k]
        assert bool((d["text_ids_masked"][b, slots] == 103).all()) and bool((slots > 0).all())
        atts = d["text_atts"][b]
        assert bool((atts[torch.arange(L), torch.arange(L)] == 1).all())
        if not fg_free:
            assert torch.equal(atts, tri) and torch.equal(d["position_ids"][b], torch.arange(L))
            continue
        want = tri.clone()
        want[:, slots] = 0
        want[slots, slots] = 1
        assert torch.equal(atts, want)
        pid = d["position_ids"][b]
        assert torch.equal(pid[slots], pid[slots + 1])                  # a [MASK] and its token share a position
        assert torch.equal(d["text_ids_masked"][b, slots + 1], d["masked_ids"][b, :k])
        assert bool((pid[1:] >= pid[:-1]).all())


def smoothed_from_chunks(z, labels, w, V, ignore, ls, chunk=64):
    """The fused kernels' form: per 64-column chunk (max, sum exp, sum z), z at the label and at the ignored class, then
    KL = sum q log q - s (sum z - z_t - z_ign) - conf z_t + sum(q) lse."""
    R = z.shape[0]
    zc = torch.nn.functional.pad(z, (0, (-V) % chunk), value=float("-inf")).view(R, -1, chunk)
    mx = zc.max(-1).values
    se = torch.exp(zc - mx.unsqueeze(-1)).sum(-1)
    sz = torch.where(torch.isinf(zc), torch.zeros_like(zc), zc).sum(-1)
    M = mx.max(-1).values
    lse = M + torch.log((se * torch.exp(mx - M.unsqueeze(-1))).sum(-1))
    conf, s = 1.0 - ls, ls / (V - 2)
    qsum = conf + s * (V - 2)
    qlogq = conf * torch.log(torch.tensor(conf, dtype=z.dtype)) + (V - 2) * s * torch.log(torch.tensor(s, dtype=z.dtype))
    zt, zi = z[torch.arange(R), labels], z[:, ignore]
    kl = qlogq - s * (sz.sum(-1) - zt - zi) - conf * zt + qsum * lse
    kl = torch.where(labels == ignore, torch.zeros_like(kl), kl)
    return (kl * w / (w.sum() + 1e-5)).sum()


@pytest.mark.parametrize("V", [512, 30522])
def test_smoothed_loss_chunk_form_matches_definition(V):
    """Derivation check of the identity x2_ls_combine evaluates (no package code: the kernels themselves are pinned in
    test_captioning_kernels_gpu.py, the model in test_captioning_golden_cpu.py / _gpu.py)."""
    g = torch.Generator().manual_seed(V)
    R, ignore, ls = 30, 101, 0.1
    z = torch.randn(R, V, generator=g, dtype=torch.float64) * 3
    labels = torch.randint(0, V, (R,), generator=g)
    labels[::4] = ignore
    w = (labels != ignore).double()
    w[5] = 0.0
    q = torch.full((R, V), ls / (V - 2), dtype=torch.float64)
    q[:, ignore] = 0
    q.scatter_(1, labels.view(-1, 1), 1.0 - ls)
    q[labels == ignore] = 0
    kl = torch.nn.functional.kl_div(torch.log_softmax(z, -1), q, reduction="none").sum(-1)
    want = (kl * w / (w.sum() + 1e-5)).sum()
    assert abs(float(smoothed_from_chunks(z, labels, w, V, ignore, ls) - want)) < 1e-10 * max(1.0, abs(float(want)))
