"""XVLMForClassification and XVLMForVQAClassification on the HIP path against the REAL reference's run (tests/golden/<case>_cls.npz,
make_golden_cls.py: CPU fp32, eval mode, same seeded weights and batch): the six cases of cases_cls.CLS_CASES.

Bounds.  Logits: absolute error.  Loss: relative.  Gradient norms, normalised as tests/test_model_gpu.py does: per tensor
|norm - golden| / max(golden, 1e-2 x the golden total), and the total's relative error.  The path is deterministic (no atomics), so each bound is
1.5 x the worst value measured on the MI355X, rounded up.  The generator keeps every row's best logit MARGIN = 0.02 above the second best; the
logits bound has to stay below half of that, 0.01, so that bf16 operand error cannot flip an argmax - then pred and ClassificationAccuracy must
equal the golden's exactly, on every row.

Measured on the MI355X (printed by the tests; tiny_vqacls / large_shallow_vqacls / tiny_cls / tiny_video_cls / tiny_text_cls / tiny_image_cls):
  logits, absolute          9.02e-4 / 5.41e-4 / 8.14e-4 / 7.72e-4 / 8.91e-4 / 4.60e-4      (bound 1.4e-3)
  loss, relative            2.36e-5 / 9.31e-6 / 8.63e-6 / 5.64e-6 / 6.59e-6 / 5.44e-6      (bound 3.6e-5)
  worst tensor norm         1.01e-2 / 1.44e-3 / 7.55e-3 / 5.15e-3 / 2.93e-3 / 1.48e-3      (bound 1.6e-2)
  total norm                7.22e-4 / 7.27e-5 / 1.74e-3 / 2.39e-3 / 6.98e-4 / 1.00e-3      (bound 3.6e-3)
  KL mode (tiny_vqacls)     loss 3.38e-6 relative, total norm 6.34e-4: under the loss and total bounds above
  pred and ClassificationAccuracy: the golden's, exactly."""
import importlib
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cases_cls import CLS_CASES, MARGIN, cls_batch, cls_config

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
# 1.5 x the worst measured value (docstring), rounded up
BOUND = dict(logits=1.4e-3, loss=3.6e-5, gradnorm=1.6e-2, total=3.6e-3)
assert BOUND["logits"] < MARGIN / 2


def to_dev(b):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}


def loss_args(cc, b):
    return dict(targets=b["targets"], k=b["k"], weights=b["weights"]) if cc["model"] == "vqa" else dict(targets=b["targets"])


def norms_of(model, recorded):
    out = {}
    for n, p in model.named_parameters():
        if n not in recorded:                                # a single-tower branch: the other tower has no gradient in the reference either
            assert p.grad is None or not bool(p.grad.any()), "gradient for a parameter the branch does not use: " + n
            continue
        assert p.grad is not None, "no gradient for " + n
        assert bool(torch.isfinite(p.grad).all()), n
        out[n] = float(p.grad.double().norm())
    return out


@pytest.fixture(scope="module", params=list(CLS_CASES))
def run(request, synthetic, tmp_path_factory):
    """Model, golden and the runs every test reads (computed once per case and left unchanged)."""
    name = request.param
    cc = CLS_CASES[name]
    mcl = importlib.import_module("x2-vlm_amd.model_classification")
    cls = mcl.XVLMForVQAClassification if cc["model"] == "vqa" else mcl.XVLMForClassification
    model = cls(cls_config(name, str(tmp_path_factory.mktemp(name))))
    synthetic.synth_state_dict(model, cc["wseed"])
    model = model.to(dev).eval()
    g = np.load("%s/%s_cls.npz" % (GOLD_DIR, name))
    recorded = set(k[len("gradnorm/"):] for k in g.files if k.startswith("gradnorm/"))
    b = to_dev(cls_batch(synthetic, name))
    kw = loss_args(cc, b)
    loss = model(b["image"], b["text_ids"], b["text_atts"], train=True, **kw)
    loss.backward()
    norms = norms_of(model, recorded)
    model.zero_grad(set_to_none=True)
    out = dict(name=name, cc=cc, g=g, model=model, b=b, loss=float(loss.detach()), norms=norms)
    with torch.no_grad():
        prediction = model(b["image"], b["text_ids"], b["text_atts"], train=False)
        out["loss2"] = float(model(b["image"], b["text_ids"], b["text_atts"], train=True, **kw))
        if cc["model"] == "vqa":
            loss_rl, logits_rl = model(b["image"], b["text_ids"], b["text_atts"], train=True, return_logits=True, **kw)
            out["rl"] = (float(loss_rl), logits_rl.cpu())
    if "loss_kl" in g.files:
        loss_kl = model(b["image"], b["text_ids"], b["text_atts"], train=True, answer_pred=b["answer_pred"])
        loss_kl.backward()
        out["kl"] = (float(loss_kl.detach()), sum(v * v for v in norms_of(model, recorded).values()) ** 0.5)
        model.zero_grad(set_to_none=True)
    acc = mcl.ClassificationAccuracy()
    pred = acc.update(prediction, torch.from_numpy(g["acc_targets"]))
    acc2 = mcl.ClassificationAccuracy()                       # the golden's accuracy is 0 for random targets: a second count with known hits
    half = torch.from_numpy(np.where(np.arange(len(g["pred"])) % 2 == 0, g["pred"], -100))
    acc2.update(prediction, half)
    torch.cuda.synchronize()
    out.update(prediction=prediction.cpu(), pred=pred.cpu(), acc=acc, acc2=acc2)
    return out


def test_logits_and_loss_match_the_reference(run):
    g = run["g"]
    e_e = float(np.abs(run["prediction"].numpy() - g["logits"]).max())
    e_l = abs(run["loss"] - float(g["loss"])) / float(g["loss"])
    print("cls %s: train=False logits %.3e absolute (bound %.1e); loss rel %.3e (bound %.1e)" % (run["name"], e_e, BOUND["logits"], e_l, BOUND["loss"]))
    assert run["prediction"].shape == g["logits"].shape and run["prediction"].dtype == torch.float32
    assert e_e <= BOUND["logits"] and e_l <= BOUND["loss"]
    assert run["loss2"] == run["loss"]                                   # deterministic: the same bits from a second forward


def test_gradient_norms_match_the_reference(run):
    g = run["g"]
    total = float(g["total_grad_norm"])
    worst, worst_name = 0.0, ""
    for n, v in run["norms"].items():
        ref = float(g["gradnorm/" + n])
        e = abs(v - ref) / max(ref, 1e-2 * total)
        if e > worst:
            worst, worst_name = e, n
    e_t = abs(sum(v * v for v in run["norms"].values()) ** 0.5 - total) / total
    print("cls %s: worst per-tensor norm error %.3e (%s; bound %.1e), total norm %.3e (bound %.1e)"
          % (run["name"], worst, worst_name, BOUND["gradnorm"], e_t, BOUND["total"]))
    assert len(run["norms"]) == sum(1 for k in g.files if k.startswith("gradnorm/"))          # every parameter the reference trains got a gradient
    assert worst <= BOUND["gradnorm"] and e_t <= BOUND["total"]


def test_predictions_and_accuracy_equal_the_reference(run):
    g = run["g"]
    assert run["pred"].dtype == torch.int32 and np.array_equal(run["pred"].numpy(), g["pred"])
    res = run["acc"].result()
    assert list(res) == ["acc"] and res["acc"] == float(g["acc"])
    assert run["acc"].formatted() == {"acc": "{:.4f}".format(float(g["acc"]))}
    n = len(g["pred"])
    assert run["acc2"].result()["acc"] == ((n + 1) // 2) / n


def test_return_logits_and_the_kl_loss(run):
    g = run["g"]
    if run["cc"]["model"] != "vqa":
        assert "rl" not in run and "loss_rl" not in g.files
        return
    loss_rl, logits_rl = run["rl"]
    assert loss_rl == run["loss"] and torch.equal(logits_rl, run["prediction"])               # the pair of return_logits=True: the same launches
    assert abs(loss_rl - float(g["loss_rl"])) <= BOUND["loss"] * float(g["loss_rl"])
    if "kl" in run:
        loss_kl, total_kl = run["kl"]
        e_k = abs(loss_kl - float(g["loss_kl"])) / float(g["loss_kl"])
        e_t = abs(total_kl - float(g["total_grad_norm_kl"])) / float(g["total_grad_norm_kl"])
        print("cls %s: KL loss rel %.3e (bound %.1e), its total gradient norm %.3e (bound %.1e)" % (run["name"], e_k, BOUND["loss"], e_t, BOUND["total"]))
        assert e_k <= BOUND["loss"] and e_t <= BOUND["total"]


def test_the_loss_is_the_reference_formula_on_the_same_logits(run):
    """recomputed in float64 from the logits of the same run: the ignored target leaves the mean (XVLMForClassification), the row count stays the
    denominator and a row without answers adds nothing (XVLMForVQAClassification)"""
    cc, b = run["cc"], run["b"]
    l = run["prediction"].double()
    if cc["model"] == "vqa":
        rows = torch.repeat_interleave(torch.arange(l.shape[0]), torch.tensor(b["k"]))
        nll = F.cross_entropy(l[rows], b["targets"].cpu(), ignore_index=-100, reduction="none")
        want = float((b["weights"].cpu().double() * nll).sum() / l.shape[0])
    else:
        want = float(F.cross_entropy(l, b["targets"].cpu(), ignore_index=-100))
    assert abs(run["loss"] - want) <= 1e-5 * want, (run["loss"], want)


def test_few_labels_take_the_register_tail(synthetic, tmp_path):
    """num_labels <= 16 goes through ops.cls_tail: its loss is F.cross_entropy on its own logits, with one ignored target"""
    mcl = importlib.import_module("x2-vlm_amd.model_classification")
    model = mcl.XVLMForClassification(dict(cls_config("tiny_cls", str(tmp_path)), num_labels=10))
    synthetic.synth_state_dict(model, CLS_CASES["tiny_cls"]["wseed"])
    model = model.to(dev).eval()
    b = to_dev(cls_batch(synthetic, "tiny_cls"))
    targets = torch.tensor([3, 9, -100, 0], device=dev)
    loss = model(b["image"], b["text_ids"], b["text_atts"], targets, train=True)
    loss.backward()
    with torch.no_grad():
        prediction = model(b["image"], b["text_ids"], b["text_atts"], train=False)
    want = float(F.cross_entropy(prediction.double().cpu(), targets.cpu(), ignore_index=-100))
    assert prediction.shape == (4, 10) and abs(float(loss) - want) <= 1e-5 * want
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    reg = mcl.XVLMForClassification(dict(cls_config("tiny_cls", str(tmp_path)), num_labels=1)).to(dev)
    with pytest.raises(NotImplementedError, match="regression"):
        reg(b["image"], b["text_ids"], b["text_atts"], torch.zeros(4, device=dev), train=True)
