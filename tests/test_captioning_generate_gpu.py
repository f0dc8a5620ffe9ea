"""XVLMForMLMCaptioning.generate / beam_search on the HIP path against the REAL reference's beam search (tests/golden/<case>_captioning_generate.npz,
make_golden_captioning_generate.py: CPU fp32, same seeded weights and image), tiny and base_shallow (V = 30522).

The reference's token choices cannot be reproduced bit for bit in bf16 - the gap between its K-th and (K+1)-th candidate goes down to 5e-4,
below the bf16 score error - so the comparison is teacher-forced: with the reference's selections fed back (_forced), every step's [MASK]-row
log-scores must be within 2 x 1.5e-2 x (the step's max-abs logit in the golden) of the reference's.  1.5e-2 of max-abs is the bound
test_captioning_golden_gpu.py holds these very scores to, and log-softmax subtracts a logsumexp whose error is at most the logits' error.
The same bound holds the cached step to the existing full-sequence forward (tril [S, L, L] mask over prompt + forced tokens + [MASK]) at every
step - the check of the cache slots, of hist and of the stale [MASK] entry.  The free-running
search must equal the host merge / back tracking replayed on its own traces exactly, may leave the reference's path only at a near-tie, and
returns the golden ids for every image that never leaves it.  "Leaves" is judged on the (id, back pointer) pairs of a step, not on the ids
alone: two beams of an image can carry the same id (tiny, image 1, last step: ids [307, 307, 2], scores -26.99548 / -26.99606), and their
swap changes the caption without changing the id list.  Where other candidates are selected, the golden's K-th minus (K+1)-th margin of
that image and step must be below twice the bound; where the same candidates come in another order - which that margin cannot see - the
golden scores of the reordered ranks must lie within twice the bound of each other.

Measured (printed by the tests): teacher-forced worst |log-score - reference| tiny 1.8e-2 (bound 6.2e-2, 0.29 of it), base_shallow 3.1e-2
(bound 1.9e-1, 0.17 of it); cached against uncached logits tiny 1.1e-2, base_shallow 3.9e-2 - two bf16 pipelines whose attention rounds
differently (the full-sequence kernel rounds the probabilities to bf16 before the second MFMA, x2_attn_decode keeps them in fp32), the
same order as either one's distance to the fp32 reference, a wrong slot would be two orders above it.  Free run: tiny image 0 and
base_shallow image 0 stay on the reference's path; tiny images 1 and 2 leave it at the last step (margins 5.7e-4 and 5.0e-4), base_shallow
image 1 at step 1 (margin 1.3e-2)."""
import importlib
import os

import numpy as np
import pytest
import torch

from cases import CASES
from cases_captioning import CAP_CASES, caption_config, write_vocab

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")
GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")
PROMPT = "w7 w9"


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("x2-vlm_amd.decode")


def setup_case(name, synthetic, workdir):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    cc = CAP_CASES[name]
    c = CASES[cc["case"]]
    g = np.load("%s/%s_captioning_generate.npz" % (GOLD_DIR, name))
    cfg = caption_config(cc["case"], str(workdir))
    cfg["prompt"] = PROMPT
    write_vocab(cfg["text_encoder"], c["vocab"])
    model = mg.XVLMForMLMCaptioning(cfg)
    assert model.prompt_ids == g["prompt_ids"].tolist() and model.generation_token_ids() == (int(g["eos_token_id"]), int(g["mask_token_id"]))
    synthetic.synth_state_dict(model, cc["wseed"])
    model = model.to(dev).eval()
    image = synthetic.synth_captioning_batch(cc["bseed"], cc["batch"], cc["max_tokens"], cc["max_masks"], c["image_res"], c["vocab"],
                                             fg_free=False)["image"].to(dev)
    B, T, Kb = image.shape[0], int(g["steps"]), int(g["num_beams"])
    length = B + int(g["max_length"])
    args = (image, torch.tensor(model.prompt_ids, device=dev).view(1, -1).expand(B, -1), torch.zeros(B, length, dtype=torch.long, device=dev),
            torch.arange(length, device=dev).view(1, -1).expand(B, -1),
            torch.tril(torch.ones(length, length, dtype=torch.long, device=dev)).view(1, length, length).expand(B, length, length))
    kw = dict(num_beams=Kb, min_length=int(g["min_length"]))
    return dict(name=name, g=g, model=model, image=image, args=args, kw=kw, B=B, T=T, K=Kb, V=c["vocab"],
                bound=[2 * 1.5e-2 * float(g["maxabs_%d" % t]) for t in range(T)])


@pytest.fixture(scope="module", params=["tiny", "base_shallow"])
def run(request, synthetic, tmp_path_factory):
    """Model, golden and the three searches every test reads (computed once per case and left unchanged): teacher-forced with the cache,
    teacher-forced through the full-sequence forward, free-running."""
    out = setup_case(request.param, synthetic, tmp_path_factory.mktemp(request.param))
    g, T, model = out["g"], out["T"], out["model"]
    forced = ([g["step_ids_%d" % t] for t in range(T)], [g["back_ptrs_%d" % t] for t in range(T)])
    out["forced"] = model.beam_search(*out["args"], **out["kw"], _forced=forced, _return_traces=True)
    out["uncached"] = model.beam_search(*out["args"], **out["kw"], _forced=forced, _return_traces=True, _use_cache=False)
    out["free"] = model.beam_search(*out["args"], **out["kw"], _return_traces=True)
    return out


def forced_sequences(g, t, B, Kb):
    """ids of every beam row before step t on the golden's path (what the n-gram rule of step t sees)"""
    seqs = [[] for _ in range(B * Kb)]
    for u in range(t):
        ids, back = g["step_ids_%d" % u], g["back_ptrs_%d" % u]
        seqs = [(seqs[b * Kb + int(back[b, k])] if u else []) + [int(ids[b, k])] for b in range(B) for k in range(Kb)]
    return seqs


def test_teacher_forced_scores_match_the_reference(run, D):
    g, B, Kb, V = run["g"], run["B"], run["K"], run["V"]
    pred, tr = run["forced"]
    for t in range(run["T"]):                                              # the run followed the reference's selections
        assert np.array_equal(tr["step_ids"][t].numpy(), g["step_ids_%d" % t]) and np.array_equal(tr["back_ptrs"][t].numpy(), g["back_ptrs_%d" % t])
    assert len(pred) == B and all(len(p) == g["output_ids"].shape[1] for p in pred)
    worst = 0.0
    for t in range(run["T"]):
        st = tr["steps"][t]
        seqs = forced_sequences(g, t, B, Kb) if t else None
        forbid = t + 1 <= int(g["min_length"])
        mine = D.log_scores_reference(st["logits"].cpu(), seqs, 3, int(g["eos_token_id"]), forbid)       # float64 from this path's logits
        ids = torch.from_numpy(g["top_ids_%d" % t]).long()
        want = torch.from_numpy(g["top_vals_%d" % t]).double()
        got = torch.gather(mine, 1, ids)
        pen = want < -5000.0
        assert torch.equal(got < -5000.0, pen), t                          # the -10000 entries compare exactly as "penalised"
        err = float((got - want)[~pen].abs().max())
        err = max(err, float((torch.logsumexp(st["logits"].cpu().double(), -1) - torch.from_numpy(g["lse_%d" % t])).abs().max()))
        if "logs_%d" % t in g:                                             # V = 512: every column, and the kernel's own penalised log-scores
            full = torch.from_numpy(g["logs_%d" % t]).double()
            klogs = st["logs"].cpu().double()
            pen = full < -5000.0
            assert torch.equal(klogs < -5000.0, pen), t
            err = max(err, float((klogs - full)[~pen].abs().max()))
        # what x2_logprob_topk returned is the top-K of this path's own scores
        order = torch.sort(mine, dim=1, descending=True, stable=True).indices[:, :Kb]
        kv, ki = st["vals"].cpu().double(), st["ids"].cpu().long()
        assert float((kv - torch.gather(mine, 1, ki)).abs().max()) <= 1e-4 and float((kv - torch.gather(mine, 1, order)).abs().max()) <= 1e-4, t
        worst = max(worst, err / run["bound"][t])
        print("teacher-forced %s step %d: worst |log-score - reference| %.3e (bound %.3e)" % (run["name"], t, err, run["bound"][t]))
        assert err <= run["bound"][t], (t, err)
    print("teacher-forced %s: worst error / bound %.3f" % (run["name"], worst))


def test_cached_step_matches_the_full_sequence_forward(run):
    a, b = run["forced"][1]["steps"], run["uncached"][1]["steps"]
    worst = 0.0
    for t in range(run["T"]):
        err = float((a[t]["logits"].double() - b[t]["logits"].double()).abs().max())
        worst = max(worst, err)
        print("cached vs uncached %s step %d: worst |logit difference| %.3e (bound %.3e)" % (run["name"], t, err, run["bound"][t]))
        assert err <= run["bound"][t], (t, err)
    print("cached vs uncached %s: worst %.3e" % (run["name"], worst))


def test_free_run_is_the_host_replay_and_leaves_the_reference_only_at_near_ties(run, D):
    g, B, Kb, T = run["g"], run["B"], run["K"], run["T"]
    pred, tr = run["free"]
    eos = int(g["eos_token_id"])
    last_scores = last_eos = None
    sc, ids, ptr = [], [], []
    for t in range(T):
        st = tr["steps"][t]
        k_scores, k_ids, back, _ = D.merge_beams(st["vals"].cpu(), st["ids"].cpu(), last_scores, last_eos, Kb)
        assert torch.equal(k_ids, tr["step_ids"][t]) and torch.equal(back, tr["back_ptrs"][t]) and torch.equal(k_scores, tr["total_scores"][t]), t
        sc.append(k_scores.tolist()); ids.append(k_ids.tolist()); ptr.append(back.tolist())
        last_scores, last_eos = k_scores, (k_ids == eos).to(k_scores.dtype)
    assert D.backtrace(sc, ids, ptr, eos, 0, len(pred[0])) == pred
    for b in range(B):
        gold_sel = [list(zip(g["step_ids_%d" % t][b].tolist(), g["back_ptrs_%d" % t][b].tolist())) for t in range(T)]
        mine_sel = [list(zip(ids[t][b], ptr[t][b])) for t in range(T)]
        first = next((t for t in range(T) if mine_sel[t] != gold_sel[t]), None)
        if first is None:
            assert pred[b] == g["output_ids"][b].tolist(), b
            print("free run %s image %d: on the reference's path, output %s" % (run["name"], b, pred[b]))
            continue
        allowed = 2 * run["bound"][first]
        if sorted(mine_sel[first]) != sorted(gold_sel[first]):             # another candidate got in: the K-th / (K+1)-th margin
            rows = [b] if first == 0 else list(range(b * Kb, (b + 1) * Kb))
            margin = min(float(g["margin1_%d" % first][rows].min()), float(g["margin2_%d" % first][b]))
            what = "selects other candidates"
        else:                                                              # the same candidates in another order: the band of their golden scores
            moved = [k for k in range(Kb) if mine_sel[first][k] != gold_sel[first][k]]
            band = g["total_scores_%d" % first][b][moved]
            margin = float(band.max() - band.min())
            what = "orders ranks %s differently" % moved
        print("free run %s image %d: leaves the reference's path at step %d (%s), golden margin %.3e (allowed below %.3e)"
              % (run["name"], b, first, what, margin, allowed))
        assert margin < allowed, (b, first, margin)


def test_generate_surface(synthetic, tmp_path):
    run = setup_case("tiny", synthetic, tmp_path)
    model, image, g = run["model"], run["image"], run["g"]
    gen = dict(num_beams=run["K"], max_length=int(g["max_length"]), min_length=int(g["min_length"]))
    model.train()
    flags = [p.requires_grad for p in model.parameters()]
    caps = model.generate(image, **gen)
    assert model.training and [p.requires_grad for p in model.parameters()] == flags
    model.eval()
    assert len(caps) == run["B"] and all(isinstance(c, str) for c in caps)
    assert caps == model.generate(image, **gen)                             # two calls, identical output (train mode above: no dropout site)
    assert caps == [model.tokenizer.decode(ids, skip_special_tokens=True) for ids in model.beam_search(*run["args"], **run["kw"])]
    one = model.generate(image, num_beams=1, max_length=6, min_length=2)
    assert len(one) == run["B"] and all(isinstance(c, str) for c in one)
    single = model.generate(image[:1], **gen)
    assert len(single) == 1 and isinstance(single[0], str)
    with pytest.raises(NotImplementedError, match="follow-up"):
        model.generate(image.cpu())
    with pytest.raises(ValueError, match="max_position_embeddings"):
        model.generate(image, max_length=64)
