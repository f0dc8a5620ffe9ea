"""XVLMForVQA.forward(train=True) on the HIP path against the REAL reference's training step (tests/golden/<case>_vqa_train.npz,
make_golden_vqa_train.py: CPU fp32, eval mode, same seeded weights and batch), tiny and base_shallow (V = 30522): the loss, the per-answer
losses (a forward hook on text_decoder, as the generator records them), every parameter's gradient norm, the total norm and a 64-element sample
of the decoder word embeddings' gradient at rows the answers use - the tied parameter, where the lookup and the LM head both contribute.

Bounds.  Loss and per-answer losses: relative.  Gradient norms, normalised as tests/step_helpers.py does: per tensor |norm - golden| /
max(golden, 1e-2 x the golden total), key biases left out (analytically zero, rounding noise in the reference); the total's relative error.
The sample: error over the sample's max-abs.  Each bound is 1.5 x the worst value measured on the MI355X, rounded up, and none is above the
loosest bound the project holds a comparable path to (loss 2e-3, per tensor 1.5e-2, sample 5e-2: tests/test_captioning_golden_gpu.py; total
3.6e-3: tests/test_cls_wide_golden_gpu.py).

Measured on the MI355X (printed by the tests; tiny / base_shallow):
  loss, relative            1.47e-4 / 6.18e-5      (bound 2.2e-4)
  worst per-answer loss     7.35e-4 / 4.83e-4      (bound 1.2e-3)
  worst tensor norm         5.65e-3 / 3.12e-3      (bound 8.5e-3)
  total norm                1.01e-3 / 1.62e-3      (bound 2.5e-3)
  word-embedding sample     5.27e-3 / 6.11e-3      (bound 9.2e-3)
  with the tied head's word-embedding gradient dropped: that tensor's norm 0.77 / 0.60, total norm 8.0e-2 / 2.2e-2, sample 1.0 / 1.0
  three padding rows: loss and every gradient tensor bit for bit; a row moved to the next question: its loss moves by 4.9e-2 / 4.3e-2 relative

Beyond the golden: a list k and a device k give the same bits; three all-padding rows behind sum(k) (ids 0, attention 0, weight 1.0 - the row
kernel zeroes it) leave the loss within 1e-6 relative and every gradient tensor within step_helpers' 5e-3, nothing NaN or inf; permuting the
rows of one question (weights alike) moves the loss by at most 1e-6 relative, while moving a row to the next question changes that row's loss and
no other row's; dropping the tied head's word-embedding gradient (a monkeypatched kernels.gemm_tn_grouped) fails the gradient check; weights
gets no gradient; answer ranking gives the same bits before and after a training call and sees weights updated through p.data after one."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cases_vqa_train import VQA_TRAIN_CASES, WORD, vqa_train_batch, vqa_train_config, word_sample_index

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
# 1.5 x the worst measured value (docstring), rounded up; ceilings: loss / answer 2e-3, gradnorm 1.5e-2, total 3.6e-3, sample 5e-2
BOUND = dict(loss=2.2e-4, answer=1.2e-3, gradnorm=8.5e-3, total=2.5e-3, sample=9.2e-3)
assert BOUND["loss"] <= 2e-3 and BOUND["answer"] <= 2e-3 and BOUND["gradnorm"] <= 1.5e-2 and BOUND["total"] <= 3.6e-3 and BOUND["sample"] <= 5e-2


def build(name, synthetic, workdir):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    model = mg.XVLMForVQA(vqa_train_config(name, str(workdir)))
    synthetic.synth_state_dict(model, VQA_TRAIN_CASES[name]["wseed"])
    return model.to(dev).eval()


def to_dev(b):
    return {k: v.to(dev) for k, v in b.items()}


def train_call(model, b, k, weights=None, ids=None, atts=None):
    """one training forward + backward from clean gradients -> (loss fp32 scalar (detached), answer_loss [S], {name: gradient})"""
    q = SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"])
    a = SimpleNamespace(input_ids=b["answer_ids"] if ids is None else ids, attention_mask=b["answer_atts"] if atts is None else atts)
    model.zero_grad(set_to_none=True)
    seen = []
    hook = model.text_decoder.register_forward_hook(lambda m, i, o: seen.append(o))
    try:
        loss = model(b["image"], q, a, k=k, weights=b["weights"] if weights is None else weights, train=True)
    finally:
        hook.remove()
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad and len(seen) == 1
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss.detach().clone(), seen[0].loss.detach().clone(), grads


def gradient_errors(grads, g, answer_ids):
    """(worst per-tensor norm error and its name, total norm error, sample error) of gradients {name: tensor} against golden g"""
    total = float(g["total_grad_norm"])
    worst, worst_name, sq = 0.0, "", 0.0
    for n, t in grads.items():
        assert bool(torch.isfinite(t).all()), n
        v = float(t.double().norm())
        sq += v * v
        if n.endswith("key.bias"):
            continue
        ref = float(g["gradnorm/" + n])
        e = abs(v - ref) / max(ref, 1e-2 * total)
        if e > worst:
            worst, worst_name = e, n
    gw = grads[WORD].double().cpu()
    idx = torch.tensor(word_sample_index(answer_ids.cpu(), gw.shape[1]))
    want = torch.from_numpy(g["word_sample"]).double()
    e_s = float((gw.reshape(-1)[idx] - want).abs().max() / want.abs().max())
    return worst, worst_name, abs(sq ** 0.5 - total) / total, e_s


def check_gradients(name, grads, g, answer_ids):
    worst, worst_name, e_t, e_s = gradient_errors(grads, g, answer_ids)
    print("vqa train %s: worst per-tensor norm error %.3e (%s; bound %.1e), total norm %.3e (bound %.1e), word-embedding sample %.3e (bound %.1e)"
          % (name, worst, worst_name, BOUND["gradnorm"], e_t, BOUND["total"], e_s, BOUND["sample"]))
    assert worst <= BOUND["gradnorm"] and e_t <= BOUND["total"] and e_s <= BOUND["sample"]


def tensor_differences(grads, ref):
    """worst |difference| of two gradient dicts per tensor, relative to max(its norm, 1e-2 x the norm of all) - step_helpers' measure"""
    total = sum(float(t.double().pow(2).sum()) for t in ref.values()) ** 0.5
    worst = 0.0
    for n, t in ref.items():
        assert bool(torch.isfinite(grads[n]).all()), n
        if "key.bias" not in n:
            worst = max(worst, float((grads[n].double() - t.double()).norm()) / max(float(t.double().norm()), 1e-2 * total))
    return worst


@pytest.fixture(scope="module", params=list(VQA_TRAIN_CASES))
def run(request, synthetic, tmp_path_factory):
    """Model, golden and the reference run every test reads (computed once per case and left unchanged)."""
    name = request.param
    model = build(name, synthetic, tmp_path_factory.mktemp(name))
    g = np.load("%s/%s_vqa_train.npz" % (GOLD_DIR, name))
    b = to_dev(vqa_train_batch(synthetic, name))
    k = VQA_TRAIN_CASES[name]["k"]
    loss, answer_loss, grads = train_call(model, b, k)
    torch.cuda.synchronize()
    return dict(name=name, model=model, g=g, b=b, k=k, loss=loss, answer_loss=answer_loss, grads=grads)


def test_loss_and_answer_losses_match_the_reference(run):
    g = run["g"]
    e_l = abs(float(run["loss"]) - float(g["loss"])) / float(g["loss"])
    rel = np.abs(run["answer_loss"].double().cpu().numpy() - g["answer_loss"]) / np.abs(g["answer_loss"])
    print("vqa train %s: loss %.6f (reference %.6f) rel %.3e (bound %.1e); worst per-answer loss rel %.3e (bound %.1e)"
          % (run["name"], float(run["loss"]), float(g["loss"]), e_l, BOUND["loss"], float(rel.max()), BOUND["answer"]))
    assert e_l <= BOUND["loss"] and float(rel.max()) <= BOUND["answer"]
    # the reference's formula on this path's own per-answer losses
    want = float((run["b"]["weights"].double() * run["answer_loss"].double()).sum() / run["b"]["image"].shape[0])
    assert abs(float(run["loss"]) - want) <= 1e-6 * want


def test_gradients_match_the_reference(run):
    g = run["g"]
    recorded = sorted(k[len("gradnorm/"):] for k in g.files if k.startswith("gradnorm/"))
    assert sorted(run["grads"]) == recorded                                   # every parameter the reference trains got a gradient
    check_gradients(run["name"], run["grads"], g, run["b"]["answer_ids"])
    assert not run["b"]["weights"].requires_grad and run["b"]["weights"].grad is None


def test_dropping_the_tied_head_gradient_fails_the_check(run, monkeypatch):
    """the gate sees the tied contribution: without the LM head's word-embedding gradient the gradient check must fail"""
    K = importlib.import_module("x2-vlm_amd.kernels")
    real = K.gemm_tn_grouped
    dropped = []

    def without_dword(problems, *a, **kw):
        out = real(problems, *a, **kw)
        for p in problems:
            if len(p) == 5 and p[2].shape == run["grads"][WORD].shape:           # (dl, tb, dword, Vp, Hd) of engine._lm_head_backward
                p[2].zero_()
                dropped.append(p[2])
        return out
    monkeypatch.setattr(K, "gemm_tn_grouped", without_dword)
    _, _, grads = train_call(run["model"], run["b"], run["k"])
    monkeypatch.undo()
    assert len(dropped) == 1
    with pytest.raises(AssertionError):
        check_gradients(run["name"] + " (tied head gradient dropped)", grads, run["g"], run["b"]["answer_ids"])
    others = {n: t for n, t in grads.items() if n != WORD}
    assert tensor_differences(others, {n: run["grads"][n] for n in others}) <= 1e-6     # nothing else moved


def test_list_k_and_device_k_give_the_same_bits(run):
    for dtype in (torch.int64, torch.int32):
        loss, answer_loss, grads = train_call(run["model"], run["b"], torch.tensor(run["k"], dtype=dtype, device=dev))
        assert torch.equal(loss, run["loss"]) and torch.equal(answer_loss, run["answer_loss"])
        assert all(torch.equal(grads[n], t) for n, t in run["grads"].items())


def test_padding_rows_change_nothing(run):
    b, k = run["b"], run["k"]
    S, La = b["answer_ids"].shape
    ids = torch.cat([b["answer_ids"], torch.zeros(3, La, dtype=torch.int64, device=dev)])
    atts = torch.cat([b["answer_atts"], torch.zeros(3, La, dtype=torch.int64, device=dev)])
    weights = torch.cat([b["weights"], torch.ones(3, device=dev)])
    loss, answer_loss, grads = train_call(run["model"], b, torch.tensor(k, device=dev), weights=weights, ids=ids, atts=atts)
    e_l = abs(float(loss) - float(run["loss"])) / float(run["loss"])
    worst = tensor_differences(grads, run["grads"])
    print("vqa train %s with three padding rows: loss rel %.3e (bound 1e-6), worst gradient tensor difference %.3e (bound 5e-3)" % (run["name"], e_l, worst))
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(answer_loss).all()) and sorted(grads) == sorted(run["grads"])
    assert bool((answer_loss[S:] == 0).all()) and torch.equal(answer_loss[:S], run["answer_loss"])
    assert e_l <= 1e-6 and worst <= 5e-3


def test_question_states_are_shared_per_question(run):
    b, k = run["b"], run["k"]
    # inside one question's range the order of the rows means nothing
    n0 = next(i for i, n in enumerate(k) if n >= 2)
    lo = sum(k[:n0])
    perm = torch.arange(b["answer_ids"].shape[0], device=dev)
    perm[lo:lo + k[n0]] = torch.arange(lo + k[n0] - 1, lo - 1, -1, device=dev)
    loss, answer_loss, _ = train_call(run["model"], b, k, weights=b["weights"][perm].contiguous(), ids=b["answer_ids"][perm].contiguous(),
                                      atts=b["answer_atts"][perm].contiguous())
    assert abs(float(loss) - float(run["loss"])) <= 1e-6 * float(run["loss"])
    assert float(((answer_loss - run["answer_loss"][perm]).abs() / run["answer_loss"][perm]).max()) <= 1e-6
    # the last row of question n0 handed to the next question: its loss changes, no other row's does
    moved = lo + k[n0] - 1
    k2 = list(k)
    k2[n0] -= 1
    k2[n0 + 1] += 1
    _, answer_loss2, _ = train_call(run["model"], b, k2)
    rel = abs(float(answer_loss2[moved]) - float(run["answer_loss"][moved])) / float(run["answer_loss"][moved])
    print("vqa train %s: row %d under question %d instead of %d: its loss moves by %.3e relative" % (run["name"], moved, n0 + 1, n0, rel))
    assert rel > 1e-4                                                          # the path is deterministic: an unshared row would not move at all
    keep = torch.arange(answer_loss2.numel(), device=dev) != moved
    assert torch.equal(answer_loss2[keep], run["answer_loss"][keep])


def test_ranking_is_unchanged_by_training_and_sees_updated_weights(synthetic, tmp_path):
    engine = importlib.import_module("x2-vlm_amd.engine")
    model = build("tiny", synthetic, tmp_path)
    b = to_dev(vqa_train_batch(synthetic, "tiny"))
    q = SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"])
    a = SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"])          # the answer rows as the closed answer list
    before = model(b["image"], q, a, k=4, train=False)
    train_call(model, b, VQA_TRAIN_CASES["tiny"]["k"])
    assert engine.BANK.backward_seen                                           # the next forward re-casts the bf16 copies
    after = model(b["image"], q, a, k=4, train=False)
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1]) and not after[1].requires_grad
    _, _, grads = train_call(model, b, VQA_TRAIN_CASES["tiny"]["k"])
    with torch.no_grad():                                                      # an optimizer that writes through p.data: no version bump
        for n, p in model.named_parameters():
            p.data.add_(grads[n], alpha=-0.5)
    moved = model(b["image"], q, a, k=4, train=False)
    assert not torch.equal(before[1], moved[1])
