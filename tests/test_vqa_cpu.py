"""CPU checks of VQA answer ranking (XVLMForVQA, csrc/vqa.hip): the module tree has the reference's state-dict names and shapes
(tests/golden/<case>_vqa.npz lists what the real reference model had), the decoder's head is tied to the decoder's own embeddings, the
constructor keeps the reference's contract (init_params in its three configurations, its assertions, no RoBERTa), train=True and CPU input are
refused, load_pretrained maps a pre-training checkpoint's keys exactly as the reference does (recorded (key <- source) lists, decoder as deep
as the cross layers and half as deep; is_eval=True changes nothing), the host tie-rule functions the GPU tests use as references reproduce the
golden's own selections, synth_vqa_batch is deterministic with distinct rows, and the library exports the three new entry points under ABI 14."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cases import CASES
from cases_vqa import MAP_FORMS, PER_TOKEN, VQA_CASES, first_stage, pretrain_state, second_stage, vqa_batch, vqa_config

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def mg():
    return importlib.import_module("x2-vlm_amd.model_generation")


def gold(name):
    return np.load("%s/%s_vqa.npz" % (GOLD_DIR, name))


@pytest.mark.parametrize("name", ["tiny", "base_shallow"])
def test_state_dict_names_and_shapes_match_the_reference(mg, name, tmp_path):
    model = mg.XVLMForVQA(vqa_config(name, str(tmp_path)))
    g = gold(name)
    mine = sorted((n, ",".join(map(str, t.shape))) for n, t in model.state_dict().items())
    assert mine == list(zip(g["sd_names"].tolist(), g["sd_shapes"].tolist()))
    dec = model.text_decoder
    assert dec.config.fusion_layer == 0 and dec.config.num_hidden_layers == VQA_CASES[name]["num_dec_layers"]
    assert dec.config.encoder_width == dec.config.hidden_size and model.text_encoder.config.encoder_width == 768
    assert all(layer.has_cross_attention for layer in dec.bert.encoder.layer)


def test_decoder_head_is_tied_to_the_decoder_embeddings(mg, tmp_path):
    model = mg.XVLMForVQA(vqa_config("tiny", str(tmp_path)))
    dec = model.text_decoder
    assert dec.cls.predictions.decoder.weight is dec.bert.embeddings.word_embeddings.weight
    assert dec.cls.predictions.decoder.bias is dec.cls.predictions.bias
    assert dec.cls.predictions.decoder.weight.data_ptr() != model.text_encoder.embeddings.word_embeddings.weight.data_ptr()
    assert not hasattr(model.text_encoder, "cls")                              # the question encoder is the bare BertModel
    names = [n for n, _ in model.named_parameters()]
    assert "text_decoder.bert.embeddings.word_embeddings.weight" in names and "text_decoder.cls.predictions.decoder.weight" not in names


def test_init_params_in_the_three_configurations(mg, tmp_path):
    # tiny: the question width (128) differs from the vision width (768): the decoder's cross-attention K/V cannot come from the checkpoint
    model = mg.XVLMForVQA(vqa_config("tiny", str(tmp_path)))
    dec_names = ["text_decoder." + n for n, _ in model.text_decoder.named_parameters()]
    kv = [n for n in dec_names if "crossattention.self.key" in n or "crossattention.self.value" in n]
    assert len(kv) == 2 * 4 and model.init_params == kv
    model = mg.XVLMForVQA(dict(vqa_config("tiny", str(tmp_path)), large_lr_for_dec=True))
    assert model.init_params == dec_names
    # base_shallow: both widths 768
    model = mg.XVLMForVQA(vqa_config("base_shallow", str(tmp_path)))
    assert model.init_params == [] and model.dec_encoder_width == model.cross_encoder_width == 768
    assert model.pad_token_id == 0 and model.num_text_layers == 2 and model.num_cross_layers == 1


def test_constructor_assertions(mg, tmp_path):
    cfg = vqa_config("tiny", str(tmp_path))
    with pytest.raises(AssertionError):
        mg.XVLMForVQA(dict(cfg, pad_token_id="0"))
    with pytest.raises(AssertionError, match="initialization not implemented"):
        mg.XVLMForVQA(dict(cfg, num_dec_layers=3))
    assert mg.XVLMForVQA(dict(cfg, num_dec_layers=1)).text_decoder.config.num_hidden_layers == 1        # half of the two cross layers
    with pytest.raises(NotImplementedError, match="RoBERTa"):
        mg.XVLMForVQA(dict(cfg, text_encoder="data/roberta-base"))


def test_training_and_host_tensors_are_refused(mg, synthetic, tmp_path):
    model = mg.XVLMForVQA(vqa_config("tiny", str(tmp_path)))
    b = vqa_batch(synthetic, "tiny")
    q = SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"])
    a = SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"])
    with pytest.raises(NotImplementedError, match="training step"):
        model(b["image"], q, a, k=[1, 1, 1], weights=torch.ones(3))
    with pytest.raises(NotImplementedError, match="HIP path"):
        model(b["image"], q, a, k=8, train=False)
    with pytest.raises(NotImplementedError, match="HIP path"):
        model.rank_answer(torch.zeros(3, 8, 128), b["question_atts"], b["answer_ids"], b["answer_atts"], 8)
    with pytest.raises(NotImplementedError, match="labels"):
        model.text_decoder(b["answer_ids"], labels=b["answer_ids"])


def mapping_case(mg, synthetic, form, workdir):
    mp = importlib.import_module("x2-vlm_amd.model_pretrain")
    layers, fusion_at, dec_layers = MAP_FORMS[form]
    cfg = vqa_config("tiny", workdir, text_layers=layers, fusion_at=fusion_at, num_dec_layers=dec_layers)
    model = mg.XVLMForVQA(cfg)
    pre = mp.XVLM(config=dict(cfg), load_vision_params=False, load_text_params=False)
    state = pretrain_state(synthetic, [(n, tuple(t.shape)) for n, t in pre.state_dict().items() if t.is_floating_point()])
    return model, cfg, state


@pytest.mark.parametrize("form", ["full", "half"])
def test_load_pretrained_maps_keys_as_the_reference(mg, synthetic, form, tmp_path):
    model, cfg, state = mapping_case(mg, synthetic, form, str(tmp_path))
    ckpt = str(tmp_path / "pretrain.th")
    torch.save({"model": state}, ckpt)
    source = {t.numpy().tobytes(): n for n, t in state.items()}
    seen = {}
    real = model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: (seen.update(sd), real(sd, strict=strict))[1]
    msg = model.load_pretrained(ckpt, cfg, is_eval=False)
    pairs = sorted([key, source[t.numpy().tobytes()]] for key, t in seen.items() if not key.startswith("vision_encoder."))
    want = gold("tiny")["map_" + form].tolist()
    assert pairs == want
    # what that means: the decoder's layers come from the upper text-encoder layers (every second one in the halved form)
    src = dict(pairs)
    first = {"full": 2, "half": 3}[form]
    assert src["text_decoder.bert.encoder.layer.0.attention.self.query.weight"] == "text_encoder.bert.encoder.layer.%d.attention.self.query.weight" % first
    assert src["text_decoder.bert.embeddings.word_embeddings.weight"] == "text_encoder.bert.embeddings.word_embeddings.weight"
    assert src["text_encoder.encoder.layer.0.output.dense.weight"] == "text_encoder.bert.encoder.layer.0.output.dense.weight"
    assert not any("crossattention.self.key" in k or "crossattention.self.value" in k for k in src if k.startswith("text_decoder."))
    missing = [k for k in msg.missing_keys if "position_ids" not in k and "relative_position_index" not in k]
    assert sorted(missing) == sorted(model.init_params + ["text_decoder.cls.predictions.decoder.bias"])
    assert torch.equal(model.text_decoder.bert.encoder.layer[1].output.dense.weight,
                       state["text_encoder.bert.encoder.layer.%d.output.dense.weight" % {"full": 3, "half": 5}[form]])
    # the pure mapping leaves the tensors themselves alone
    again = model.map_pretrained_state(dict(state), cfg["text_encoder"])
    assert all(again[k] is state[s] for k, s in pairs)


def test_load_pretrained_is_eval_takes_the_checkpoint_as_it_is(mg, tmp_path):
    model = mg.XVLMForVQA(vqa_config("tiny", str(tmp_path)))
    own = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()}
    ckpt = str(tmp_path / "vqa.th")
    torch.save({"model": own}, ckpt)
    seen = {}
    real = model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: (seen.update(sd), real(sd, strict=strict))[1]
    msg = model.load_pretrained(ckpt, vqa_config("tiny", str(tmp_path)), is_eval=True)
    assert list(seen) == list(own) and not msg.missing_keys and not msg.unexpected_keys
    assert float(model.text_decoder.cls.predictions.bias[3]) == 0.25


@pytest.mark.parametrize("name", ["tiny", "base_shallow"])
def test_golden_is_consistent_with_the_host_tie_rules(name):
    g = gold(name)
    k = int(g["k"])
    B, Na = g["logp_first"].shape
    assert g["stage1_ids"].shape == (B, k) and g["scores"].shape == (B, k) and g["answer_loss"].shape == (B * k,)
    vals, ids = first_stage(g["logp_first"], k)
    srt = -np.sort(-g["logp_first"].astype(np.float64), axis=1)
    for b in range(B):
        assert set(ids[b].tolist()) == set(g["stage1_ids"][b].tolist())       # the same candidates; inside a tie group torch's order is its own
        assert srt[b, k - 1] > srt[b, k]                                      # the cut is not inside a tie group
        groups = [ids[b][vals[b] == v].tolist() for v in np.unique(vals[b])]
        assert all(grp == sorted(grp) for grp in groups)                     # lowest candidate index first among equals
    assert np.allclose(srt[:, k - 1] - srt[:, k], g["cut_margin"], atol=1e-5)
    assert (g["cut_margin"] > 4 * PER_TOKEN * float(g["maxabs0"])).all()
    want_logp = np.take_along_axis(g["logp_first"].astype(np.float64), g["stage1_ids"], 1)
    assert np.abs(want_logp - g["stage1_logp"]).max() <= 1e-5
    assert np.abs(g["stage1_logp"] - g["answer_loss"].reshape(B, k) - g["scores"]).max() <= 1e-5
    probs, top = second_stage(g["scores"], g["stage1_ids"])
    assert np.array_equal(top, g["topk_ids"]) and np.abs(probs - g["topk_probs"]).max() <= 1e-6
    assert np.abs(probs.sum(1) - 1).max() <= 1e-12
    srt2 = -np.sort(-g["scores"].astype(np.float64), axis=1)
    assert np.allclose(srt2[:, 0] - srt2[:, 1], g["final_margin"], atol=1e-5)


def test_host_tie_rules_on_constructed_ties():
    lp = np.array([[-1.0, -0.5, -1.0, -0.5, -3.0, -0.5]])
    vals, ids = first_stage(lp, 5)
    assert ids.tolist() == [[1, 3, 5, 0, 2]] and vals.tolist() == [[-0.5, -0.5, -0.5, -1.0, -1.0]]
    probs, top = second_stage(np.array([[-2.0, -1.0, -2.0, -1.0]]), np.array([[7, 5, 3, 9]]))
    assert top.tolist() == [[5, 9, 7, 3]] and probs[0, 0] == probs[0, 1] > probs[0, 2] == probs[0, 3]


def test_synth_vqa_batch_is_deterministic_with_distinct_rows(synthetic):
    for name, vc in VQA_CASES.items():
        a, b = vqa_batch(synthetic, name), vqa_batch(synthetic, name)
        assert all(torch.equal(a[k], b[k]) for k in a)
        c = CASES[vc["case"]]
        ids, atts = a["answer_ids"], a["answer_atts"]
        Na, La = vc["n_answers"], vc["answer_len"]
        assert ids.shape == (Na, La) and a["question_ids"].shape == (vc["batch"], vc["seq_len"]) and a["image"].shape[0] == vc["batch"]
        assert len(set(map(tuple, ids.tolist()))) == Na                       # distinct rows
        firsts = set(ids[:, 1].tolist())
        assert abs(len(firsts) - Na / 3) <= 1 and len(firsts) < Na            # candidates share first tokens
        lens = atts.sum(1)
        assert int(lens.min()) >= 3 and int(lens.max()) == La and len(set(lens.tolist())) > 1
        sep = 102 if c["vocab"] > 2000 else 2
        assert bool((ids[:, 0] == ids[0, 0]).all()) and bool((ids.gather(1, (lens - 1).view(-1, 1)) == sep).all())
        assert bool(((ids == 0) == (atts == 0)).all()) and (a["question_atts"] == 0).any()
    other = vqa_batch(synthetic, "tiny", aseed=VQA_CASES["tiny"]["aseed"] + 1)
    assert not torch.equal(other["answer_ids"], vqa_batch(synthetic, "tiny")["answer_ids"])
    with pytest.raises(ValueError):
        synthetic.synth_vqa_batch(1, 2, 8, 32, 512, 40, 3)


def test_library_exports_the_vqa_entry_points():
    lib = importlib.import_module("x2-vlm_amd._lib")
    K = importlib.import_module("x2-vlm_amd.kernels")
    h = lib.lib()
    for name in ("x2_answer_topk", "x2_vqa_candidates", "x2_vqa_rerank"):
        assert name in lib.EXPORTS and hasattr(h, name)
    assert h.x2_abi_version() == 14
    for fn in ("answer_topk", "vqa_candidates", "vqa_rerank", "mlm_ce_rows"):
        assert callable(getattr(K, fn))
    # the limits are refused before anything is dereferenced or launched (no GPU here)
    import ctypes
    one = ctypes.c_void_p(16)
    assert h.x2_answer_topk(one, 512, 512, 1, one, 300, 257, one, one, None) == -1 and b"x2_answer_topk" in h.x2_last_error()
    assert h.x2_answer_topk(one, 512, 512, 1, one, 7, 8, one, one, None) == -1
    assert h.x2_answer_topk(one, 512, 512, 1, one, 65537, 8, one, one, None) == -1
    assert h.x2_answer_topk(one, 512, 512, 1, one, 7, 0, one, one, None) == -1
    assert h.x2_vqa_candidates(one, one, one, 40, 129, 2, 8, 0, one, one, one, one, 192, None) == -1 and b"La=129" in h.x2_last_error()
    assert h.x2_vqa_candidates(one, one, one, 40, 5, 2, 8, 0, one, one, one, one, 5, None) == -1
    assert h.x2_vqa_rerank(one, 7, one, one, 2, 257, one, one, one, None) == -1 and b"x2_vqa_rerank" in h.x2_last_error()
    assert h.x2_vqa_rerank(one, 128, one, one, 2, 8, one, one, one, None) == -1
