"""XVLMForVQA.forward(train=False) / rank_answer on the HIP path against the REAL reference's answer ranking (tests/golden/<case>_vqa.npz,
make_golden_vqa.py: CPU fp32, same seeded weights and batch), tiny and base_shallow (V = 30522).

Bound: the project's rule for log-scores (tests/test_captioning_generate_gpu.py): 2 x 1.5e-2 x maxabs0 per scored token, maxabs0 the golden's
max-abs first-step logit.  The first-step logsumexp and every answer's first-token log-probability are held to one token's bound; a
candidate's score to that times its number of scored tokens - the first token (stage 1) plus every label the candidate pass scores.

Teacher-forced (the golden's stage-1 ids fed to the second stage): lse0, logp_first and the scores against the golden.  Free run: the
first stage must select the golden's candidates as a set per question (inside a tie group the order is the kernel's rule, torch's is its
own; the generator keeps the cut out of tie groups and more than four bounds wide), the best answer must be the golden's wherever the
golden's final margin exceeds twice the bound - with per-candidate bounds: wherever the best score leads every other candidate j by more
than bound(best) + bound(j), see decided_by - (at most one question per case may fall below), the probabilities sum to 1.  The unfused path
(_fused=False: logits materialised, torch bookkeeping) gives the same best answers and scores within the same bound on tiny, and two
copies of one image and question give identical rows - K/V sharing and the per-question kernels do not mix questions.

Measured (printed by the tests): teacher-forced worst |logp_first - reference| tiny 9.3e-3 (bound 7.4e-2), base_shallow 2.3e-2 (bound 1.8e-1);
worst |score - reference| / bound tiny 0.046, base_shallow 0.088; free run: the reference's candidates and best answers for all five questions;
fused against unfused scores on tiny 1e-5 of the bound."""
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cases_vqa import PER_TOKEN, VQA_CASES, vqa_batch, vqa_config

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


def setup_case(name, synthetic, workdir):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    vc = VQA_CASES[name]
    g = np.load("%s/%s_vqa.npz" % (GOLD_DIR, name))
    model = mg.XVLMForVQA(vqa_config(name, str(workdir)))
    synthetic.synth_state_dict(model, vc["wseed"])
    model = model.to(dev).eval()
    b = {k: v.to(dev) for k, v in vqa_batch(synthetic, name).items()}
    q = SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"])
    a = SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"])
    k = vc["k"]
    assert int(g["k"]) == k
    ntok = b["answer_atts"].sum(1).cpu().numpy().astype(np.float64)            # scored tokens of an answer: its first token twice over
    #   (once in stage 1, once as the candidate pass's first label) plus the rest up to [SEP] = 1 + (length - 1)
    return dict(name=name, g=g, model=model, image=b["image"], q=q, a=a, k=k, B=vc["batch"], per_token=PER_TOKEN * float(g["maxabs0"]), ntok=ntok)


def decided_by(scores, bounds):
    """"final_margin exceeds twice the bound" with per-candidate bounds (a candidate's bound grows with its scored tokens): the least, over
    the other candidates j, of (best score - score j) - (bound of the best + bound of j).  Positive: no admissible error pair can put
    another candidate first.  With equal bounds this is final_margin - 2 x bound."""
    best = int(np.argmax(scores))
    return float(min((scores[best] - scores[j]) - (bounds[best] + bounds[j]) for j in range(len(scores)) if j != best))


@pytest.fixture(scope="module", params=["tiny", "base_shallow"])
def run(request, synthetic, tmp_path_factory):
    """Model, golden and the runs every test reads (computed once per case and left unchanged)."""
    out = setup_case(request.param, synthetic, tmp_path_factory.mktemp(request.param))
    m, k = out["model"], out["k"]
    out["forced"] = m(out["image"], out["q"], out["a"], k=k, train=False, _stage1_ids=out["g"]["stage1_ids"], _return_traces=True)
    out["free"] = m(out["image"], out["q"], out["a"], k=k, train=False, _return_traces=True)
    torch.cuda.synchronize()
    return out


def test_teacher_forced_scores_match_the_reference(run):
    g, tr, per = run["g"], run["forced"][2], run["per_token"]
    lse = torch.logsumexp(tr["logits0"].double(), -1).cpu().numpy()
    e_lse = float(np.abs(lse - g["lse0"]).max())
    e_first = float(np.abs(tr["logp_first"].double().cpu().numpy() - g["logp_first"]).max())
    assert np.array_equal(tr["stage1_ids"].cpu().numpy(), g["stage1_ids"])
    bound = per * run["ntok"][g["stage1_ids"]]
    err = np.abs(tr["scores"].double().cpu().numpy() - g["scores"])
    loss_err = float(np.abs(tr["loss_rows"].double().sum(1).cpu().numpy() - g["answer_loss"]).max())
    print("teacher-forced %s: |lse0 - ref| %.3e, worst |logp_first - ref| %.3e (bound %.3e, %.3f of it); worst |score - ref| %.3e, worst "
          "score error / bound %.3f; worst |answer loss - ref| %.3e"
          % (run["name"], e_lse, e_first, per, max(e_lse, e_first) / per, float(err.max()), float((err / bound).max()), loss_err))
    assert e_lse <= per and e_first <= per
    assert bool((err <= bound).all()), float((err / bound).max())


def test_free_run_selects_the_reference_candidates_and_answers(run):
    g, per, B, k = run["g"], run["per_token"], run["B"], run["k"]
    ids, probs, tr = run["free"]
    assert ids.shape == (B, k) and ids.dtype == torch.int64 and probs.shape == (B, k) and probs.dtype == torch.float32
    s1 = tr["stage1_ids"].cpu().numpy()
    below = 0
    for b in range(B):
        assert set(s1[b].tolist()) == set(g["stage1_ids"][b].tolist()), b
        assert sorted(ids[b].tolist()) == sorted(s1[b].tolist())                # the re-ranking permutes the selected candidates
        slack = decided_by(g["scores"][b], per * run["ntok"][g["stage1_ids"][b]])
        if slack > 0:
            assert int(ids[b, 0]) == int(g["topk_ids"][b, 0]), b
        else:
            below += 1
        print("free run %s question %d: best answer %d (reference %d), reference margin %.3e, least (gap - the two candidates' bounds) %.3e"
              % (run["name"], b, int(ids[b, 0]), int(g["topk_ids"][b, 0]), float(g["final_margin"][b]), slack))
    assert below <= 1
    assert float((probs.double().sum(1) - 1).abs().max()) <= 1e-5
    assert bool((probs[:, :-1] >= probs[:, 1:]).all())
    # inside a tie group of the first stage the lower candidate index comes first
    v = tr["stage1_logp"].cpu().numpy()
    for b in range(B):
        assert all(v[b, j] > v[b, j + 1] or (v[b, j] == v[b, j + 1] and s1[b, j] < s1[b, j + 1]) for j in range(k - 1))


def test_unfused_path_agrees(synthetic, tmp_path):
    run = setup_case("tiny", synthetic, tmp_path)
    m, k = run["model"], run["k"]
    ids_f, probs_f, tr_f = m(run["image"], run["q"], run["a"], k=k, train=False, _return_traces=True)
    ids_u, probs_u, tr_u = m(run["image"], run["q"], run["a"], k=k, train=False, _fused=False, _return_traces=True)
    assert torch.equal(ids_f[:, 0], ids_u[:, 0])
    worst = 0.0
    for b in range(run["B"]):
        sf = dict(zip(tr_f["stage1_ids"][b].tolist(), tr_f["scores"][b].tolist()))
        su = dict(zip(tr_u["stage1_ids"][b].tolist(), tr_u["scores"][b].tolist()))
        assert set(sf) == set(su)
        for cand in sf:
            err = abs(sf[cand] - su[cand])
            worst = max(worst, err / (run["per_token"] * run["ntok"][cand]))
            assert err <= run["per_token"] * run["ntok"][cand], (b, cand, err)
    assert float((probs_u.double().sum(1) - 1).abs().max()) <= 1e-5
    print("fused vs unfused tiny: worst |score difference| / bound %.3e" % worst)


def test_copies_of_one_question_give_identical_rows(synthetic, tmp_path):
    run = setup_case("tiny", synthetic, tmp_path)
    m, k = run["model"], run["k"]
    image = run["image"][1:2].repeat(2, 1, 1, 1)
    q = SimpleNamespace(input_ids=run["q"].input_ids[1:2].repeat(2, 1), attention_mask=run["q"].attention_mask[1:2].repeat(2, 1))
    ids, probs = m(image, q, run["a"], k=k, train=False)
    assert torch.equal(ids[0], ids[1]) and torch.equal(probs[0], probs[1])
    free = m(run["image"], run["q"], run["a"], k=k, train=False)
    assert int(ids[0, 0]) == int(free[0][1, 0])                                 # and the answer that question gets in the full batch


def test_forward_surface(synthetic, tmp_path):
    run = setup_case("tiny", synthetic, tmp_path)
    m, k = run["model"], run["k"]
    m.train()
    flags = [p.requires_grad for p in m.parameters()]
    ids, probs = m(run["image"], run["q"], run["a"], k=k, train=False)
    assert m.training and [p.requires_grad for p in m.parameters()] == flags and not probs.requires_grad
    m.eval()
    again = m(run["image"], run["q"], run["a"], k=k, train=False)
    assert torch.equal(ids, again[0]) and torch.equal(probs, again[1])          # train mode above: no dropout site
    one = m(run["image"], run["q"], run["a"], k=1, train=False)
    assert one[0].shape == (run["B"], 1) and torch.equal(one[1], torch.ones_like(one[1]))
    full = m(run["image"][:1], SimpleNamespace(input_ids=run["q"].input_ids[:1], attention_mask=run["q"].attention_mask[:1]), run["a"],
             k=run["a"].input_ids.shape[0], train=False)
    assert sorted(full[0][0].tolist()) == list(range(run["a"].input_ids.shape[0]))
    with pytest.raises(ValueError, match="rank_answer"):
        m(run["image"], run["q"], run["a"], k=run["a"].input_ids.shape[0] + 1, train=False)
    with pytest.raises(NotImplementedError, match="training step"):
        m(run["image"], run["q"], run["a"], k=[1], weights=torch.ones(1, device=dev))
