"""CPU checks of the NLVR2 fine-tune (XVLMForNLVR, csrc/classify.hip): the module tree has the reference's state-dict names, shapes and
init_params (tests/golden/<case>_nlvr.npz lists what the real reference model had); the inherited load_pretrained maps a pre-training
checkpoint's keys exactly as the reference does (recorded (key <- source) list); host tensors are refused; the library exports the three new
entry points under ABI 14 and refuses R, H, C, a leading dimension or an alignment outside the documented ranges without a launch; the oracle's
existing functions, composed as the reference composes its stages (cross_embeds(text_ids=...) twice, head_mlp on the concatenated CLS rows,
cross_entropy), reproduce the golden logits and loss; the generator's margin condition holds for the committed fixtures.

Oracle bound.  Both sides are fp32 on the CPU and differ only in summation order.  Measured worst case over the three cases (printed below):
logits 4.84e-8 absolute, loss 5.96e-8 absolute - one ulp (2^-24) of a loss in [0.5, 1).  The bound is 1.5 x the worst, rounded up to whole ulps
of the loss: 2 x 2^-24 = 1.2e-7, far below the 1e-5 ceiling."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from cases import CASES
from cases_nlvr import MARGIN, NLVR_CASES, logit_margin, nlvr_batch, nlvr_config, pretrain_state
from oracle import x2vlm_oracle as O

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
ORACLE_BOUND = 1.2e-7
assert ORACLE_BOUND <= 1e-5


@pytest.fixture(scope="module")
def mcl():
    return importlib.import_module("x2-vlm_amd.model_classification")


def gold(name):
    return np.load("%s/%s_nlvr.npz" % (GOLD_DIR, name))


@pytest.mark.parametrize("name", ["tiny", "large_shallow"])
def test_constructor_contract_matches_the_reference(mcl, name, tmp_path):
    model = mcl.XVLMForNLVR(nlvr_config(name, str(tmp_path)))
    g = gold(name)
    mine = sorted((n, ",".join(map(str, t.shape))) for n, t in model.state_dict().items())
    assert mine == list(zip(g["sd_names"].tolist(), g["sd_shapes"].tolist()))
    assert model.init_params == g["init_params"].tolist()
    assert model.init_params == ["cls_head.0.weight", "cls_head.0.bias", "cls_head.1.weight", "cls_head.1.bias", "cls_head.3.weight", "cls_head.3.bias"]
    W = model.text_width
    assert tuple(model.cls_head[0].weight.shape) == (4 * W, 2 * W) and tuple(model.cls_head[3].weight.shape) == (2, 4 * W)
    assert model.cls_head[1].eps == 1e-5
    assert not model.use_bbox_loss and not model.use_contrastive_loss and not model.use_matching_loss
    assert not hasattr(model.text_encoder, "cls") and not hasattr(model, "itm_head") and not hasattr(model, "bbox_head")
    assert sorted(n for n, _ in model.named_parameters()) == sorted(k[len("gradnorm/"):] for k in g.files if k.startswith("gradnorm/"))


def test_load_pretrained_maps_keys_as_the_reference(mcl, synthetic, tmp_path):
    mp = importlib.import_module("x2-vlm_amd.model_pretrain")
    cfg = nlvr_config("tiny", str(tmp_path))
    model = mcl.XVLMForNLVR(cfg)
    before = model.cls_head[3].weight.detach().clone()
    pre = mp.XVLM(config=dict(cfg), load_vision_params=False, load_text_params=False)
    state = pretrain_state(synthetic, [(n, tuple(t.shape)) for n, t in pre.state_dict().items() if t.is_floating_point()])
    ckpt = str(tmp_path / "pretrain.th")
    torch.save({"model": state}, ckpt)
    source = {t.numpy().tobytes(): n for n, t in state.items()}
    seen = {}
    real = model.load_state_dict
    model.load_state_dict = lambda sd, strict=True: (seen.update(sd), real(sd, strict=strict))[1]
    msg = model.load_pretrained(ckpt, cfg, is_eval=False)
    pairs = sorted([key, source[t.numpy().tobytes()]] for key, t in seen.items() if not key.startswith("vision_encoder."))
    assert pairs == gold("tiny")["map_pairs"].tolist()
    src = dict(pairs)
    assert src["text_encoder.encoder.layer.3.crossattention.self.key.weight"] == "text_encoder.bert.encoder.layer.3.crossattention.self.key.weight"
    assert sorted(k for k in msg.missing_keys if "position_ids" not in k and "relative_position_index" not in k) == sorted(model.init_params)
    assert "itm_head.0.weight" in msg.unexpected_keys and "temp" in msg.unexpected_keys
    assert torch.equal(model.cls_head[3].weight, before)                      # the head is trained from scratch
    assert torch.equal(model.text_encoder.encoder.layer[1].output.dense.weight, state["text_encoder.bert.encoder.layer.1.output.dense.weight"])
    assert sorted(model.init_params) == sorted("cls_head." + n for n, _ in model.cls_head.named_parameters())


def test_host_tensors_are_refused(mcl, synthetic, tmp_path):
    ops = importlib.import_module("x2-vlm_amd.ops")
    model = mcl.XVLMForNLVR(nlvr_config("tiny", str(tmp_path)))
    b = nlvr_batch(synthetic, "tiny")
    for train in (True, False):
        with pytest.raises(NotImplementedError, match="HIP path"):
            model(b["image"], b["text_ids"], b["text_atts"], b["targets"], train=train)
    with pytest.raises(NotImplementedError, match="HIP path"):
        ops.cls_tail(model.cls_head, torch.zeros(4, model.cls_head[1].weight.numel()), b["targets"])
    with pytest.raises(NotImplementedError, match="HIP path"):
        mcl.NLVRAccuracy().update(torch.zeros(4, 2), b["targets"])


def test_library_exports_the_classification_entry_points():
    lib = importlib.import_module("x2-vlm_amd._lib")
    K = importlib.import_module("x2-vlm_amd.kernels")
    ops = importlib.import_module("x2-vlm_amd.ops")
    h = lib.lib()
    for name in ("x2_cls_tail_fwd", "x2_cls_tail_bwd", "x2_cls_accuracy"):
        assert name in lib.EXPORTS and hasattr(h, name) and getattr(h, name).argtypes is not None
    assert h.x2_abi_version() == 14
    for fn in ("cls_tail_fwd", "cls_tail_bwd", "cls_accuracy"):
        assert callable(getattr(K, fn))
    assert callable(ops.cls_tail)


def test_argument_checks_refuse_without_launching():
    """every check returns before anything is dereferenced or launched (no GPU here)"""
    h = importlib.import_module("x2-vlm_amd._lib").lib()
    one, odd = ctypes.c_void_p(16), ctypes.c_void_p(20)

    def fwd(R=8, H=256, C=2, ldh=None, hp=one, gp=one, bp=one, wp=one, labels=one, nll=one, stat=one, logits=one):
        return h.x2_cls_tail_fwd(hp, H if ldh is None else ldh, gp, bp, wp, one, labels, R, H, C, 1e-5, logits, one, nll, stat, None)

    def bwd(R=8, H=256, C=2, ldh=None, lddh=None, hp=one, gp=one, bp=one, wp=one, dh=one, labels=one, stat=one, g_loss=one, dw=one):
        return h.x2_cls_tail_bwd(hp, H if ldh is None else ldh, gp, bp, wp, one, one, labels, stat, g_loss, None, R, H, C, dh,
                                 H if lddh is None else lddh, one, one, dw, one, None)

    def acc(R=8, C=2, logits=one, counts=one):
        return h.x2_cls_accuracy(logits, one, R, C, one, counts, None)

    def refused(rc, name, word=None):
        msg = h.x2_last_error()
        assert rc == -1 and name in msg and (word is None or word in msg), (rc, msg)

    for R in (0, -1, 65537):
        refused(fwd(R=R), b"x2_cls_tail_fwd", b"R=")
        refused(bwd(R=R), b"x2_cls_tail_bwd", b"R=")
        refused(acc(R=R), b"x2_cls_accuracy", b"R=")
    for H in (0, 2, 6, 255, 16388, 32768):
        refused(fwd(H=H), b"x2_cls_tail_fwd", b"H=")
        refused(bwd(H=H), b"x2_cls_tail_bwd", b"H=")
    for C in (0, 1, 17):
        refused(fwd(C=C), b"x2_cls_tail_fwd", b"C=")
        refused(bwd(C=C), b"x2_cls_tail_bwd", b"C=")
        refused(acc(C=C), b"x2_cls_accuracy", b"C=")
    for ld in (252, 258):                                                  # below H; not a multiple of 4
        refused(fwd(ldh=ld), b"x2_cls_tail_fwd", b"ldh=")
        refused(bwd(ldh=ld), b"x2_cls_tail_bwd", b"ldh=")
        refused(bwd(lddh=ld), b"x2_cls_tail_bwd", b"lddh=")
    for kw in (dict(hp=odd), dict(gp=odd), dict(bp=odd), dict(wp=odd)):
        refused(fwd(**kw), b"x2_cls_tail_fwd", b"aligned")
        refused(bwd(**kw), b"x2_cls_tail_bwd", b"aligned")
    refused(bwd(dh=odd), b"x2_cls_tail_bwd", b"aligned")
    refused(fwd(hp=None), b"x2_cls_tail_fwd", b"null")
    refused(fwd(logits=None), b"x2_cls_tail_fwd", b"null")
    refused(fwd(nll=None), b"x2_cls_tail_fwd")                             # labels without their outputs
    refused(fwd(stat=None), b"x2_cls_tail_fwd")
    refused(bwd(dw=None), b"x2_cls_tail_bwd", b"null")
    refused(bwd(stat=None), b"x2_cls_tail_bwd", b"stat")                   # a loss cotangent needs n_valid
    refused(acc(logits=None), b"x2_cls_accuracy", b"null")
    refused(acc(counts=None), b"x2_cls_accuracy", b"null")


def oracle_params(synthetic, name):
    """The NLVR model's text encoder is a bare BertModel: its state-dict names have no `bert.` infix, and the synthetic weights are seeded by
    name (as tests/test_grounding_cpu.py does for the grounding model).  cls_head is not in the oracle's parameter table: its shapes are
    build_mlp(2W, 2)'s."""
    nc = NLVR_CASES[name]
    cfg = O.config_from_case(CASES[nc["case"]])
    sd = {}
    for pname, shape in O.parameter_shapes(cfg).items():
        if pname.startswith(("text_encoder.cls.", "itm_head.", "bbox_head.", "vision_proj.", "text_proj.")) or pname == "temp":
            continue
        sd[pname] = synthetic.synth_tensor(pname.replace("text_encoder.bert.", "text_encoder."), shape, nc["wseed"])
    W = CASES[nc["case"]]["hidden"]
    for pname, shape in (("cls_head.0.weight", (4 * W, 2 * W)), ("cls_head.0.bias", (4 * W,)), ("cls_head.1.weight", (4 * W,)),
                         ("cls_head.1.bias", (4 * W,)), ("cls_head.3.weight", (2, 4 * W)), ("cls_head.3.bias", (2,))):
        sd[pname] = synthetic.synth_tensor(pname, shape, nc["wseed"])
    return cfg, sd


@pytest.mark.parametrize("name", list(NLVR_CASES))
def test_composed_oracle_reproduces_the_golden(synthetic, name):
    cfg, sd = oracle_params(synthetic, name)
    b = nlvr_batch(synthetic, name)
    g = gold(name)
    B = b["targets"].shape[0]
    assert np.array_equal(b["targets"].numpy(), g["targets"]) and b["image"].shape[0] == 2 * B
    torch.set_num_threads(8)
    with torch.no_grad():
        image_embeds = O.vision_encoder(sd, cfg, b["image"])
        ones = torch.ones(B, image_embeds.shape[1], dtype=torch.long)
        cls = [O.cross_embeds(sd, cfg, e, ones, b["text_atts"], text_ids=b["text_ids"])[:, 0] for e in (image_embeds[:B], image_embeds[B:])]
        logits = O.head_mlp(sd, "cls_head", torch.cat(cls, dim=-1))
        loss = O.cross_entropy(logits, b["targets"])
    e_l, e_s = float(np.abs(logits.numpy() - g["logits"]).max()), abs(float(loss) - float(g["loss"]))
    print("oracle vs golden %s: logits %.2e, loss %.2e (bound %.1e)" % (name, e_l, e_s, ORACLE_BOUND))
    assert e_l <= ORACLE_BOUND and e_s <= ORACLE_BOUND
    assert np.array_equal(logits.argmax(1).numpy(), g["pred"])


def test_margin_condition_holds_for_the_committed_fixtures():
    assert MARGIN == 0.15
    for name, nc in NLVR_CASES.items():
        g = gold(name)
        B = nc["pairs"]
        m = logit_margin(g["logits"])
        assert g["logits"].shape == (B, 2) and m >= MARGIN and abs(m - float(g["logit_margin"])) < 1e-9, (name, m)
        want = np.arange(B) % 2
        if "ignore" in nc:
            want[nc["ignore"]] = -100
        assert np.array_equal(g["targets"], want)
        assert np.array_equal(g["pred"], g["logits"].argmax(1))
        assert abs(float(g["acc"]) - float((g["pred"] == g["targets"]).mean())) < 1e-7
    a, b = gold("tiny"), gold("tiny_ignore")
    assert np.array_equal(a["logits"], b["logits"]) and float(a["loss"]) != float(b["loss"])
    # the ignored row leaves the mean: the loss divides by 3, not 4
    l = a["logits"].astype(np.float64)
    nll = np.log(np.exp(l).sum(1)) - l[np.arange(4), a["targets"]]
    assert abs(nll.mean() - float(a["loss"])) < 1e-6 and abs(np.delete(nll, 1).sum() / 3 - float(b["loss"])) < 1e-6
