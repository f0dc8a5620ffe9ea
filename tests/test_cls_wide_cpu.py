"""CPU checks of the wide-label classification fine-tunes (XVLMForClassification, XVLMForVQAClassification, csrc/classify_wide.hip): the module
trees have the reference's state-dict names, shapes and init_params (tests/golden/<case>_cls.npz lists what the real reference models had); the
inherited load_pretrained maps a pre-training checkpoint's keys exactly as the reference does (recorded (key <- source) list); host tensors and
the MSE regression head are refused; ops.cls_wide names the H % 64 rule; the library exports the seven new entry points under ABI 14 and refuses
R, H, C, a leading dimension, an alignment or a NULL offs outside the documented ranges without a launch; the oracle's existing functions,
composed as the reference composes its stages, with the weighted soft cross-entropy and the KL loss written below in numpy, reproduce the golden
logits and losses; the generator's margin condition holds for the committed fixtures.

Oracle bound.  Both sides are fp32 on the CPU and differ only in summation order.  Logits: 1.2e-7 absolute, the bound of tests/test_nlvr_cpu.py
for the same arithmetic (measured worst over the six cases: printed below, 1.04e-7).  Losses: the reference's loss is an fp32 number near 7, whose
spacing is 4.8e-7, while the numpy losses below are float64 sums over the oracle's logits: the two differ by up to half an fp32 ulp of the loss
plus the logits' own error.  LOSS_BOUND is therefore relative, 1.2e-7 (two ulps, 2 x 2^-24, of a number in [0.5, 1): the same two ulps as
test_nlvr_cpu.py's bound, scaled to the loss); measured worst 3.97e-8 relative for the cross-entropies, 5.89e-8 for the KL loss."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from cases import CASES
from cases_cls import CLS_CASES, MARGIN, cls_batch, cls_config, top2_margin
from cases_nlvr import pretrain_state
from oracle import x2vlm_oracle as O

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
LOGITS_BOUND = 1.2e-7
LOSS_BOUND = 1.2e-7          # relative
HEAD = ["cls_head.0.weight", "cls_head.0.bias", "cls_head.1.weight", "cls_head.1.bias", "cls_head.3.weight", "cls_head.3.bias"]
NEW = ("x2_lngelu_fwd", "x2_lngelu_bwd", "x2_soft_ce_fwd", "x2_kl_ce_fwd", "x2_soft_ce_bwd", "x2_kl_ce_bwd", "x2_cls_accuracy_rows")


@pytest.fixture(scope="module")
def mcl():
    return importlib.import_module("x2-vlm_amd.model_classification")


def gold(name):
    return np.load("%s/%s_cls.npz" % (GOLD_DIR, name))


def build(mcl, name, workdir):
    cls = mcl.XVLMForVQAClassification if CLS_CASES[name]["model"] == "vqa" else mcl.XVLMForClassification
    return cls(cls_config(name, workdir))


@pytest.mark.parametrize("name", ["tiny_vqacls", "large_shallow_vqacls", "tiny_cls", "tiny_video_cls", "tiny_image_cls"])
def test_constructor_contract_matches_the_reference(mcl, name, tmp_path):
    model = build(mcl, name, str(tmp_path))
    g, cc = gold(name), CLS_CASES[name]
    mine = sorted((n, ",".join(map(str, t.shape))) for n, t in model.state_dict().items())
    assert mine == list(zip(g["sd_names"].tolist(), g["sd_shapes"].tolist()))
    assert list(model.init_params) == g["init_params"].tolist()
    assert list(model.init_params) == (HEAD if cc["model"] == "vqa" else [])
    F = model.vision_width if cc.get("task_name") == "imagenet" else model.text_width
    assert tuple(model.cls_head[0].weight.shape) == (2 * F, F) and tuple(model.cls_head[3].weight.shape) == (cc["labels"], 2 * F)
    assert model.cls_head[1].eps == 1e-5
    assert not model.use_bbox_loss and not model.use_contrastive_loss and not model.use_matching_loss
    assert not hasattr(model.text_encoder, "cls") and not hasattr(model, "itm_head") and not hasattr(model, "bbox_head")
    mine = set(n for n, _ in model.named_parameters())
    recorded = set(k[len("gradnorm/"):] for k in g.files if k.startswith("gradnorm/"))
    assert recorded <= mine and (recorded == mine or "branch" in cc) and set(HEAD) <= recorded


def test_load_pretrained_maps_keys_as_the_reference(mcl, synthetic, tmp_path):
    mp = importlib.import_module("x2-vlm_amd.model_pretrain")
    cfg = cls_config("tiny_vqacls", str(tmp_path))
    model = mcl.XVLMForVQAClassification(cfg)
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
    assert pairs == gold("tiny_vqacls")["map_pairs"].tolist()
    src = dict(pairs)
    assert src["text_encoder.encoder.layer.3.crossattention.self.key.weight"] == "text_encoder.bert.encoder.layer.3.crossattention.self.key.weight"
    assert sorted(k for k in msg.missing_keys if "position_ids" not in k and "relative_position_index" not in k) == sorted(model.init_params)
    assert "itm_head.0.weight" in msg.unexpected_keys and "temp" in msg.unexpected_keys
    assert torch.equal(model.cls_head[3].weight, before)                      # the head is trained from scratch
    assert torch.equal(model.text_encoder.encoder.layer[1].output.dense.weight, state["text_encoder.bert.encoder.layer.1.output.dense.weight"])
    assert sorted(model.init_params) == sorted(HEAD)
    # XVLMForClassification defines no init_params of its own: the inherited loader fills them with what the checkpoint lacked
    other = mcl.XVLMForClassification(cls_config("tiny_cls", str(tmp_path)))
    assert other.init_params == []
    other.load_pretrained(ckpt, cls_config("tiny_cls", str(tmp_path)), is_eval=False)
    assert sorted(other.init_params) == sorted(HEAD)


def test_host_tensors_and_unbuilt_heads_are_refused(mcl, synthetic, tmp_path):
    ops = importlib.import_module("x2-vlm_amd.ops")
    for name in ("tiny_vqacls", "tiny_cls", "tiny_text_cls"):
        model = build(mcl, name, str(tmp_path))
        b = cls_batch(synthetic, name)
        for train in (True, False):
            with pytest.raises(NotImplementedError, match="HIP path"):
                model(b["image"], b["text_ids"], b["text_atts"], b["targets"], train=train)
    with pytest.raises(NotImplementedError, match="HIP path"):
        ops.cls_wide(model.cls_head, torch.zeros(4, model.cls_head[1].weight.numel()))
    with pytest.raises(NotImplementedError, match="HIP path"):
        mcl.ClassificationAccuracy().update(torch.zeros(4, 1500), torch.zeros(4, dtype=torch.int64))
    reg = mcl.XVLMForClassification(dict(cls_config("tiny_cls", str(tmp_path)), num_labels=1))
    assert tuple(reg.cls_head[3].weight.shape) == (1, 256) and reg.num_labels == 1
    assert issubclass(mcl.ClassificationAccuracy, mcl.NLVRAccuracy)


def test_library_exports_the_wide_head_entry_points():
    lib = importlib.import_module("x2-vlm_amd._lib")
    K = importlib.import_module("x2-vlm_amd.kernels")
    ops = importlib.import_module("x2-vlm_amd.ops")
    h = lib.lib()
    for name in NEW:
        assert name in lib.EXPORTS and hasattr(h, name) and getattr(h, name).argtypes is not None and len(getattr(h, name).argtypes) >= 9
    assert h.x2_abi_version() == 14
    for fn in ("lngelu_fwd", "lngelu_bwd", "soft_ce_fwd", "kl_ce_fwd", "soft_ce_bwd", "kl_ce_bwd", "cls_accuracy_rows"):
        assert callable(getattr(K, fn))
    assert callable(ops.cls_wide)


def test_argument_checks_refuse_without_launching():
    """every check returns before anything is dereferenced or launched (no GPU here)"""
    h = importlib.import_module("x2-vlm_amd._lib").lib()
    one, odd, byte = ctypes.c_void_p(16), ctypes.c_void_p(20), ctypes.c_void_p(18)

    def lnf(R=8, H=256, ldh=None, lda=None, hp=one, gp=one, bp=one, act=one, rs=one):
        return h.x2_lngelu_fwd(hp, H if ldh is None else ldh, gp, bp, R, H, 1e-5, act, H if lda is None else lda, rs, None)

    def lnb(R=8, H=256, ldd=None, ldh=None, lddh=None, da=one, hp=one, gp=one, bp=one, dh=one, dg=one):
        return h.x2_lngelu_bwd(da, H if ldd is None else ldd, hp, H if ldh is None else ldh, gp, bp, one, R, H, dh, H if lddh is None else lddh,
                               dg, one, None)

    def sf(R=8, C=100, ldl=None, lg=one, offs=one, tg=one, w=one, mode=0, lse=one, rl=one, st=one):
        return h.x2_soft_ce_fwd(lg, C if ldl is None else ldl, R, C, offs, tg, w, mode, lse, rl, st, None)

    def kf(R=8, C=100, ldl=None, ldt=None, lg=one, te=one, st=one):
        return h.x2_kl_ce_fwd(lg, C if ldl is None else ldl, te, C if ldt is None else ldt, R, C, one, one, one, st, None)

    def sb(R=8, C=100, Cp=128, ldl=None, ldg=None, lddl=None, lg=one, offs=one, gl=one, glg=one, dl=one, st=one):
        return h.x2_soft_ce_bwd(lg, C if ldl is None else ldl, R, C, offs, one, one, one, st, gl, glg, C if ldg is None else ldg, dl,
                                Cp if lddl is None else lddl, Cp, None)

    def kb(R=8, C=100, Cp=128, ldl=None, ldt=None, ldg=None, lddl=None, lg=one, te=one, gl=one, glg=one, dl=one):
        return h.x2_kl_ce_bwd(lg, C if ldl is None else ldl, te, C if ldt is None else ldt, R, C, one, one, gl, glg, C if ldg is None else ldg, dl,
                              Cp if lddl is None else lddl, Cp, None)

    def acc(R=8, C=100, ldl=None, lg=one, counts=one, hit=one):
        return h.x2_cls_accuracy_rows(lg, C if ldl is None else ldl, one, R, C, one, hit, counts, None)

    def refused(rc, name, word=None):
        msg = h.x2_last_error()
        assert rc == -1 and name in msg and (word is None or word in msg), (rc, msg)

    rc_fns = dict(x2_lngelu_fwd=lnf, x2_lngelu_bwd=lnb, x2_soft_ce_fwd=sf, x2_kl_ce_fwd=kf, x2_soft_ce_bwd=sb, x2_kl_ce_bwd=kb, x2_cls_accuracy_rows=acc)
    assert sorted(rc_fns) == sorted(NEW)
    for name, fn in rc_fns.items():
        for R in (0, -1, 65537):
            refused(fn(R=R), name.encode(), b"R=")
    for H in (0, 2, 6, 255, 16388, 32768):                                 # H % 4, and the range
        refused(lnf(H=H), b"x2_lngelu_fwd", b"H=")
        refused(lnb(H=H), b"x2_lngelu_bwd", b"H=")
    for name in ("x2_soft_ce_fwd", "x2_kl_ce_fwd", "x2_soft_ce_bwd", "x2_kl_ce_bwd", "x2_cls_accuracy_rows"):
        for C in (-3, 0, 1):
            refused(rc_fns[name](C=C, **({"Cp": 64} if name.endswith("bwd") else {})), name.encode(), b"C=")
    for ld in (252, 258):                                                  # below H; not a multiple of 4
        refused(lnf(ldh=ld), b"x2_lngelu_fwd", b"ldh=")
        refused(lnf(lda=ld), b"x2_lngelu_fwd", b"lda=")
        for kw in ("ldd", "ldh", "lddh"):
            refused(lnb(**{kw: ld}), b"x2_lngelu_bwd", kw.encode() + b"=")
    refused(sf(ldl=99), b"x2_soft_ce_fwd", b"ldl=")                          # ld < C
    refused(kf(ldl=99), b"x2_kl_ce_fwd", b"ldl=")
    refused(kf(ldt=99), b"x2_kl_ce_fwd", b"ldt=")
    refused(sb(ldl=99), b"x2_soft_ce_bwd", b"ldl=")
    refused(sb(ldg=99), b"x2_soft_ce_bwd", b"ldg=")
    refused(kb(ldl=99), b"x2_kl_ce_bwd", b"ldl=")
    refused(kb(ldt=99), b"x2_kl_ce_bwd", b"ldt=")
    refused(kb(ldg=99), b"x2_kl_ce_bwd", b"ldg=")
    refused(acc(ldl=99), b"x2_cls_accuracy_rows", b"ldl=")
    for fn, name in ((sb, b"x2_soft_ce_bwd"), (kb, b"x2_kl_ce_bwd")):
        refused(fn(Cp=96), name, b"Cp=")                                   # below C
        refused(fn(Cp=102), name, b"Cp=")                                  # not a multiple of 4
        refused(fn(lddl=124), name, b"lddl=")                              # below Cp
        refused(fn(lddl=130), name, b"lddl=")
        refused(fn(dl=odd), name, b"aligned")                              # bf16 rows are written four at a time
        refused(fn(dl=None), name, b"null")
    for kw in (dict(hp=odd), dict(gp=odd), dict(bp=odd), dict(act=odd)):
        refused(lnf(**kw), b"x2_lngelu_fwd", b"aligned")
    for kw in (dict(da=odd), dict(hp=odd), dict(gp=odd), dict(bp=odd), dict(dh=odd)):
        refused(lnb(**kw), b"x2_lngelu_bwd", b"aligned")
    refused(sf(lg=byte), b"x2_soft_ce_fwd", b"aligned")
    refused(kf(lg=byte), b"x2_kl_ce_fwd", b"aligned")
    refused(acc(lg=byte), b"x2_cls_accuracy_rows", b"aligned")
    refused(sf(offs=None), b"x2_soft_ce_fwd", b"offs")                       # NULL offs
    refused(sb(offs=None), b"x2_soft_ce_bwd", b"offs")
    refused(sf(mode=2), b"x2_soft_ce_fwd", b"denom_mode=")
    refused(sf(rl=None), b"x2_soft_ce_fwd")                                  # targets without their outputs
    refused(sf(st=None), b"x2_soft_ce_fwd")
    refused(sf(tg=None), b"x2_soft_ce_fwd", b"weights")                      # weights without targets
    refused(sf(lg=None), b"x2_soft_ce_fwd", b"null")
    refused(kf(te=None), b"x2_kl_ce_fwd", b"null")
    refused(kf(st=None), b"x2_kl_ce_fwd", b"null")
    refused(sb(st=None), b"x2_soft_ce_bwd", b"stat")                         # a loss cotangent needs the denominator
    refused(kb(te=None), b"x2_kl_ce_bwd", b"teacher")
    refused(lnf(rs=None), b"x2_lngelu_fwd", b"null")
    refused(lnb(dg=None), b"x2_lngelu_bwd", b"null")
    refused(acc(counts=None), b"x2_cls_accuracy_rows", b"null")
    refused(acc(hit=None), b"x2_cls_accuracy_rows", b"null")


# ---------------------------------------------------------------------------------------------------- the composed oracle against the goldens

def soft_ce_np(logits, targets, k, weights, denom):
    """sum_b sum_j w_j (lse(logits[b]) - logits[b, t_j]) / denom over row b's k[b] entries, skipping targets outside [0, C); denom 'rows' or
    'entries' (the non-skipped ones); float64"""
    l = np.asarray(logits, dtype=np.float64)
    lse = np.log(np.exp(l - l.max(1, keepdims=True)).sum(1)) + l.max(1)
    total, n, e = 0.0, 0, 0
    for b, kb in enumerate(k):
        for _ in range(kb):
            t = int(targets[e])
            if 0 <= t < l.shape[1]:
                total += float(weights[e]) * (lse[b] - l[b, t])
                n += 1
            e += 1
    return total / (l.shape[0] if denom == "rows" else n)


def kl_np(logits, teacher):
    l, t = np.asarray(logits, dtype=np.float64), np.asarray(teacher, dtype=np.float64)
    logp = l - (np.log(np.exp(l - l.max(1, keepdims=True)).sum(1)) + l.max(1))[:, None]
    logq = t - (np.log(np.exp(t - t.max(1, keepdims=True)).sum(1)) + t.max(1))[:, None]
    q = np.exp(logq)
    return float(np.where(q > 0, q * (logq - logp), 0.0).sum() / l.shape[0])


def oracle_params(synthetic, name):
    """The fine-tune models' text encoder is a bare BertModel: its state-dict names have no `bert.` infix, and the synthetic weights are seeded by
    name.  cls_head is not in the oracle's parameter table: its shapes are build_mlp(F, C)'s."""
    cc = CLS_CASES[name]
    cfg = O.config_from_case(CASES[cc["case"]])
    sd = {}
    for pname, shape in O.parameter_shapes(cfg).items():
        if pname.startswith(("text_encoder.cls.", "itm_head.", "bbox_head.", "vision_proj.", "text_proj.")) or pname == "temp":
            continue
        sd[pname] = synthetic.synth_tensor(pname.replace("text_encoder.bert.", "text_encoder."), shape, cc["wseed"])
    F = CASES[cc["case"]].get("vision_width", 768) if cc.get("task_name") == "imagenet" else CASES[cc["case"]]["hidden"]
    C = cc["labels"]
    for pname, shape in (("cls_head.0.weight", (2 * F, F)), ("cls_head.0.bias", (2 * F,)), ("cls_head.1.weight", (2 * F,)),
                         ("cls_head.1.bias", (2 * F,)), ("cls_head.3.weight", (C, 2 * F)), ("cls_head.3.bias", (C,))):
        sd[pname] = synthetic.synth_tensor(pname, shape, cc["wseed"])
    return cfg, sd


@pytest.mark.parametrize("name", list(CLS_CASES))
def test_composed_oracle_reproduces_the_golden(synthetic, name):
    cc = CLS_CASES[name]
    cfg, sd = oracle_params(synthetic, name)
    b = cls_batch(synthetic, name)
    g = gold(name)
    assert np.array_equal(b["targets"].numpy(), g["targets"])
    torch.set_num_threads(8)
    with torch.no_grad():
        if cc.get("branch") == "text":
            cls = O.bert_encoder(sd, cfg, O.text_embeddings(sd, cfg, b["text_ids"]), b["text_atts"])[:, 0]
        else:
            image_embeds = O.frame_embeds(sd, cfg, b["image"])[0] if b["image"].dim() == 5 else O.vision_encoder(sd, cfg, b["image"])
            if cc.get("branch") == "image":
                cls = image_embeds[:, 0]
            else:
                ones = torch.ones(image_embeds.shape[:2], dtype=torch.long)
                cls = O.cross_embeds(sd, cfg, image_embeds, ones, b["text_atts"], text_ids=b["text_ids"])[:, 0]
        logits = O.head_mlp(sd, "cls_head", cls)
    B = logits.shape[0]
    if cc["model"] == "vqa":
        loss = soft_ce_np(logits.numpy(), g["targets"], g["k"], g["weights"], "rows")
        assert np.array_equal(g["k"], cc["k"]) and np.array_equal(g["weights"], b["weights"].numpy())
    else:
        loss = soft_ce_np(logits.numpy(), g["targets"], [1] * B, np.ones(B), "entries")
    e_l, e_s = float(np.abs(logits.numpy() - g["logits"]).max()), abs(loss - float(g["loss"])) / float(g["loss"])
    print("oracle vs golden %s: logits %.2e absolute (bound %.1e), loss %.2e relative (bound %.1e)" % (name, e_l, LOGITS_BOUND, e_s, LOSS_BOUND))
    assert e_l <= LOGITS_BOUND and e_s <= LOSS_BOUND
    assert np.array_equal(logits.argmax(1).numpy(), g["pred"])
    if "loss_kl" in g.files:
        e_k = abs(kl_np(logits.numpy(), b["answer_pred"].numpy()) - float(g["loss_kl"])) / float(g["loss_kl"])
        print("oracle vs golden %s: KL loss %.2e relative (bound %.1e)" % (name, e_k, LOSS_BOUND))
        assert e_k <= LOSS_BOUND
    if "loss_rl" in g.files:
        assert float(g["loss_rl"]) == float(g["loss"]) and np.array_equal(g["logits_rl"], g["logits"])


def test_margin_condition_holds_for_the_committed_fixtures():
    assert MARGIN == 0.02
    for name, cc in CLS_CASES.items():
        g = gold(name)
        B = CASES[cc["case"]]["batch"]
        m = top2_margin(g["logits"])
        assert g["logits"].shape == (B, cc["labels"]) and m >= MARGIN and abs(m - float(g["top2_margin"])) < 1e-9, (name, m)
        assert np.array_equal(g["pred"], g["logits"].argmax(1))
        assert abs(float(g["acc"]) - float((g["pred"] == g["acc_targets"]).mean())) < 1e-7
        assert os.path.getsize("%s/%s_cls.npz" % (GOLD_DIR, name)) < 1 << 20
    g = gold("tiny_vqacls")
    t, k = g["targets"], g["k"].tolist()
    assert k == [2, 0, 3, 1] and (t == -100).sum() == 1 and t[1] == -100 and t[4] == t[2] and len(t) == sum(k)
    assert set(np.round(g["weights"] * 10).astype(int).tolist()) <= set(range(1, 11))
    assert (gold("tiny_cls")["targets"] == -100).sum() == 1
    # the ignored target leaves the mean of XVLMForClassification (3 rows, not 4), and the row count stays the VQA model's denominator
    a = gold("tiny_cls")
    l = a["logits"].astype(np.float64)
    keep = a["targets"] >= 0
    nll = np.log(np.exp(l).sum(1)) - l[np.arange(4), np.where(keep, a["targets"], 0)]
    assert abs(nll[keep].sum() / 3 - float(a["loss"])) < 1e-5 and abs(nll[keep].sum() / 4 - float(a["loss"])) > 0.1
