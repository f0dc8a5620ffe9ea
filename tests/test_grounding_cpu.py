"""CPU checks of visual grounding (XVLMForGrounding, csrc/grounding.hip): the module tree has the reference's state-dict names, shapes and
init_params (tests/golden/<case>_grounding.npz lists what the real reference model had); load_pretrained maps a pre-training checkpoint's keys
exactly as the reference does (recorded (key <- source) list) and is_eval=True takes a checkpoint of this model as it is; host tensors are
refused; the library exports the three new entry points under ABI 14 and refuses a B or N outside the documented range without a launch;
the oracle's existing functions, composed as the model composes its stages, reproduce the golden coordinates and losses at the fp32 bounds
tests/test_retrieval.py holds the oracle to against a golden (2e-6 on O(1) values, 2e-5 on the derived scalars); the generator's margin condition
holds for the committed fixtures and the evaluation fixture is consistent with the float64 restatement the kernel tests use."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from cases import CASES
from cases_grounding import (EVAL_N, GROUNDING_CASES, MARGIN, SPLITS, eval_set, grounding_batch, grounding_config, iou_float64, kink_margin,
                             pretrain_state)
from oracle import x2vlm_oracle as O

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def mgr():
    return importlib.import_module("x2-vlm_amd.model_grounding")


def gold(name):
    return np.load("%s/%s_grounding.npz" % (GOLD_DIR, name))


@pytest.mark.parametrize("name", ["tiny", "large_shallow"])
def test_constructor_contract_matches_the_reference(mgr, name, tmp_path):
    model = mgr.XVLMForGrounding(grounding_config(name, str(tmp_path)))
    g = gold(name)
    mine = sorted((n, ",".join(map(str, t.shape))) for n, t in model.state_dict().items())
    assert mine == list(zip(g["sd_names"].tolist(), g["sd_shapes"].tolist()))
    assert model.init_params == g["init_params"].tolist() == []
    assert model.use_bbox_loss and not model.use_contrastive_loss and not model.use_matching_loss
    assert not hasattr(model.text_encoder, "cls") and not hasattr(model, "itm_head")          # the bare BertModel, one head
    assert sorted(n for n, _ in model.named_parameters()) == sorted(k[len("gradnorm/"):] for k in g.files if k.startswith("gradnorm/"))


def test_load_pretrained_maps_keys_as_the_reference(mgr, synthetic, tmp_path):
    mp = importlib.import_module("x2-vlm_amd.model_pretrain")
    cfg = grounding_config("tiny", str(tmp_path))
    model = mgr.XVLMForGrounding(cfg)
    pre = mp.XVLM(config=dict(cfg), load_vision_params=False, load_text_params=False)
    state = pretrain_state(synthetic, [(n, tuple(t.shape)) for n, t in pre.state_dict().items() if t.is_floating_point()])
    ckpt = str(tmp_path / "pretrain.th")
    torch.save({"model": state}, ckpt)
    source = {t.numpy().tobytes(): n for n, t in state.items()}
    seen = {}
    real = model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: (seen.update(sd), real(sd, strict=strict))[1]
    msg = model.load_pretrained(ckpt, cfg, load_bbox_pretrain=True, is_eval=False)
    pairs = sorted([key, source[t.numpy().tobytes()]] for key, t in seen.items() if not key.startswith("vision_encoder."))
    assert pairs == gold("tiny")["map_pairs"].tolist()
    src = dict(pairs)
    assert src["text_encoder.encoder.layer.3.crossattention.self.key.weight"] == "text_encoder.bert.encoder.layer.3.crossattention.self.key.weight"
    assert src["bbox_head.3.weight"] == "bbox_head.3.weight"
    assert [k for k in msg.missing_keys if "position_ids" not in k and "relative_position_index" not in k] == []
    assert "itm_head.0.weight" in msg.unexpected_keys and "temp" in msg.unexpected_keys
    assert torch.equal(model.bbox_head[3].weight, state["bbox_head.3.weight"])
    assert torch.equal(model.text_encoder.encoder.layer[1].output.dense.weight, state["text_encoder.bert.encoder.layer.1.output.dense.weight"])
    assert model.init_params == []


def test_load_pretrained_is_eval_takes_the_checkpoint_as_it_is(mgr, tmp_path):
    cfg = grounding_config("tiny", str(tmp_path))
    model = mgr.XVLMForGrounding(cfg)
    own = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()}
    ckpt = str(tmp_path / "grounding.th")
    torch.save({"model": own}, ckpt)
    seen = {}
    real = model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: (seen.update(sd), real(sd, strict=strict))[1]
    msg = model.load_pretrained(ckpt, cfg, is_eval=True)
    assert list(seen) == list(own) and not msg.missing_keys and not msg.unexpected_keys
    assert float(model.bbox_head[3].bias.detach()[2]) == 0.25


def test_host_tensors_are_refused(mgr, synthetic, tmp_path):
    model = mgr.XVLMForGrounding(grounding_config("tiny", str(tmp_path)))
    b = grounding_batch(synthetic, "tiny")
    with pytest.raises(NotImplementedError, match="HIP path"):
        model(b["image"], b["text_ids"], b["text_atts"])
    with pytest.raises(NotImplementedError, match="HIP path"):
        model(b["image"], b["text_ids"], b["text_atts"], b["target_bbox"])
    pred, ref_box, size, split = eval_set()
    with pytest.raises(NotImplementedError, match="HIP path"):
        mgr.grounding_iou(torch.from_numpy(pred), ref_box, size)
    with pytest.raises(NotImplementedError, match="HIP path"):
        mgr.grounding_eval_bbox(torch.from_numpy(pred), ref_box, size, split)


def test_library_exports_the_grounding_entry_points():
    lib = importlib.import_module("x2-vlm_amd._lib")
    K = importlib.import_module("x2-vlm_amd.kernels")
    ops = importlib.import_module("x2-vlm_amd.ops")
    h = lib.lib()
    for name in ("x2_bbox_loss_fwd", "x2_bbox_loss_bwd", "x2_grounding_iou"):
        assert name in lib.EXPORTS and hasattr(h, name)
    assert h.x2_abi_version() == 14
    for fn in ("bbox_loss_fwd", "bbox_loss_bwd", "grounding_iou"):
        assert callable(getattr(K, fn))
    assert callable(ops.bbox_loss)
    # the limits are refused before anything is dereferenced or launched (no GPU here)
    one = ctypes.c_void_p(16)
    for B in (0, -1, (1 << 20) + 1):
        assert h.x2_bbox_loss_fwd(one, one, None, B, one, one, None) == -1 and b"x2_bbox_loss_fwd" in h.x2_last_error()
        assert h.x2_bbox_loss_bwd(one, one, None, one, one, one, None, B, one, None) == -1 and b"x2_bbox_loss_bwd" in h.x2_last_error()
    for N in (0, -5, (1 << 24) + 1):
        assert h.x2_grounding_iou(one, one, one, N, one, one, None) == -1 and b"x2_grounding_iou" in h.x2_last_error()
    assert h.x2_bbox_loss_fwd(None, one, None, 4, one, one, None) == -1 and b"x2_bbox_loss_fwd" in h.x2_last_error()
    assert h.x2_bbox_loss_bwd(one, one, None, None, one, one, None, 4, one, None) == -1 and b"x2_bbox_loss_bwd" in h.x2_last_error()
    assert h.x2_grounding_iou(one, one, one, 4, one, None, None) == -1 and b"x2_grounding_iou" in h.x2_last_error()
    assert h.x2_bbox_loss_fwd(ctypes.c_void_p(20), one, None, 4, one, one, None) == -1 and b"aligned" in h.x2_last_error()


def oracle_params(synthetic, name):
    """The grounding model's text encoder is a bare BertModel: its state-dict names have no `bert.` infix, and the synthetic weights are
    seeded by name (as tests/test_retrieval.py does for the retrieval model)."""
    gc = GROUNDING_CASES[name]
    cfg = O.config_from_case(CASES[gc["case"]])
    sd = {}
    for pname, shape in O.parameter_shapes(cfg).items():
        if pname.startswith(("text_encoder.cls.", "itm_head.", "vision_proj.", "text_proj.")) or pname == "temp":
            continue
        sd[pname] = synthetic.synth_tensor(pname.replace("text_encoder.bert.", "text_encoder."), shape, gc["wseed"])
    return cfg, sd


@pytest.mark.parametrize("name", list(GROUNDING_CASES))
def test_composed_oracle_reproduces_the_golden(synthetic, name):
    cfg, sd = oracle_params(synthetic, name)
    b = grounding_batch(synthetic, name)
    g = gold(name)
    assert np.array_equal(b["target_bbox"].numpy(), g["target_bbox"])
    torch.set_num_threads(8)
    with torch.no_grad():
        image_embeds = O.vision_encoder(sd, cfg, b["image"])
        text_embeds = O.text_embeds(sd, cfg, b["text_ids"], b["text_atts"])
        ones = torch.ones(image_embeds.shape[:2], dtype=torch.long)
        cls = O.cross_embeds(sd, cfg, image_embeds, ones, b["text_atts"], text_embeds=text_embeds)[:, 0]
        coord = O.head_mlp(sd, "bbox_head", cls).sigmoid()
        loss_bbox, loss_giou = O.bbox_loss(coord, b["target_bbox"], torch.zeros(coord.shape[0], dtype=torch.long))
    e_c = float(np.abs(coord.numpy() - g["output_coord"]).max())
    e_b, e_g = abs(float(loss_bbox) - float(g["loss_bbox"])), abs(float(loss_giou) - float(g["loss_giou"]))
    print("oracle vs golden %s: coord %.2e, loss_bbox %.2e, loss_giou %.2e" % (name, e_c, e_b, e_g))
    assert e_c <= 2e-6 and e_b <= 2e-5 and e_g <= 2e-5
    assert np.array_equal(g["infer_coord"], g["output_coord"])
    if GROUNDING_CASES[name].get("degenerate"):
        assert float(loss_giou) == 0.0 and float(g["loss_giou"]) == 0.0


def test_margin_condition_holds_for_the_committed_fixtures():
    for name, gc in GROUNDING_CASES.items():
        g = gold(name)
        if gc.get("degenerate"):
            assert float(g["target_bbox"][1, 2]) == -0.25 and float(g["loss_giou"]) == 0.0
            assert float(g["total_grad_norm"]) == float(g["total_grad_norm_bbox"])
            for k in g.files:
                if k.startswith("gradnorm/"):
                    assert float(g[k]) == float(g["gradnorm_bbox/" + k[len("gradnorm/"):]])
            continue
        m = kink_margin(g["output_coord"], g["target_bbox"])
        assert m >= MARGIN and abs(m - float(g["kink_margin"])) < 1e-9, (name, m)
        assert float(g["loss_giou"]) > 0 and float(g["total_grad_norm"]) != float(g["total_grad_norm_bbox"])
    assert MARGIN == 4 * 5e-3


def test_evaluation_fixture_is_consistent():
    g = gold("tiny")
    pred, ref_box, size, split = eval_set()
    assert g["eval_iou"].shape == (EVAL_N,) and len(split) == EVAL_N
    want = iou_float64(pred, ref_box, size)
    assert np.abs(want - g["eval_iou"]).max() <= 1e-5            # the reference's own computeIoU against the float64 restatement
    assert float((np.abs(want - 0.5) > 1e-4).mean()) >= 0.95
    assert np.array_equal(g["eval_hit"], g["eval_iou"] >= 0.5)
    assert (want == 0).any() and (want > 0.8).any()              # disjoint pairs and near-matches are both in the set
    assert abs(float(g["eval_acc/score"]) - g["eval_hit"].mean()) < 1e-12
    for name in SPLITS:
        rows = np.array([s == name for s in split])
        assert rows.sum() > 0 and abs(float(g["eval_acc/%s_d" % name]) - g["eval_hit"][rows].mean()) < 1e-12
