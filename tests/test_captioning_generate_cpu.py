"""Captioning inference, host side (no GPU): the beam merge and back tracking of decode.py replayed on the REAL reference's recorded
log-scores (tests/golden/<case>_captioning_generate.npz, make_golden_captioning_generate.py) must reproduce its step ids, back pointers and
output ids exactly and its total scores to 1e-5; the length penalty against a hand-worked value; the n-gram ban rule and its float64 score
restatement on hand-made sequences; generate()'s size rule (steps = bsz + max_length - len(prompt_ids), the reference's) and its refusals."""
import ctypes
import importlib
import os

import numpy as np
import pytest
import torch

from cases import model_config

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("x2-vlm_amd.decode")


def gold(name):
    return np.load(os.path.join(GOLD_DIR, "%s_captioning_generate.npz" % name))


def replay(D, g):
    """merge_beams step by step on the golden's per-row log-scores (full rows at V = 512, the 16 best per row otherwise)."""
    K, eos = int(g["num_beams"]), int(g["eos_token_id"])
    last_scores = last_eos = None
    out = []
    for t in range(int(g["steps"])):
        if "logs_%d" % t in g:
            vals, ids = torch.topk(torch.from_numpy(g["logs_%d" % t]), K)
        else:
            vals, ids = torch.from_numpy(g["top_vals_%d" % t])[:, :K], torch.from_numpy(g["top_ids_%d" % t])[:, :K]
        k_scores, k_ids, back, _ = D.merge_beams(vals, ids, last_scores, last_eos, K)
        out.append((k_scores, k_ids, back))
        last_scores, last_eos = k_scores, (k_ids == eos).to(k_scores.dtype)
    return out


@pytest.mark.parametrize("name", ["tiny", "base_shallow"])
def test_merge_and_backtrace_reproduce_the_reference(D, name):
    g = gold(name)
    steps = replay(D, g)
    for t, (k_scores, k_ids, back) in enumerate(steps):
        assert np.array_equal(k_ids.numpy(), g["step_ids_%d" % t]), t
        assert np.array_equal(back.numpy(), g["back_ptrs_%d" % t]), t
        assert float(np.abs(k_scores.numpy() - g["total_scores_%d" % t]).max()) <= 1e-5, t
    length = g["output_ids"].shape[1]
    pred = D.backtrace([s[0].tolist() for s in steps], [s[1].tolist() for s in steps], [s[2].tolist() for s in steps], int(g["eos_token_id"]),
                       0, length)
    assert pred == g["output_ids"].tolist()
    if name == "tiny":
        assert pred[2][:3] == [199, 93, 2] and not any(pred[2][3:])          # the third image ends with EOS at its third token


def test_length_penalty_against_a_hand_worked_value(D):
    """Two steps, two beams, EOS = 2.  Frame 0: beam 1 ends (EOS) with -1.2.  Frame 1 (the last): -1.5 and -1.3.
    penalty 0: the best of {-1.2, -1.5, -1.3} is the frame-0 EOS -> [2].
    penalty 1: -1.2 / (6 / 6) = -1.2, -1.5 / (7 / 6) = -1.2857.., -1.3 / (7 / 6) = -1.1142.. -> frame 1, beam 1, whose pointer is beam 0 of
    frame 0 -> [7, 9]."""
    scores = [[[-0.5, -1.2]], [[-1.5, -1.3]]]
    ids = [[[7, 2]], [[8, 9]]]
    ptrs = [[[0, 0]], [[0, 0]]]
    assert D.backtrace(scores, ids, ptrs, 2, 0) == [[2]]
    assert D.backtrace(scores, ids, ptrs, 2, 1.0) == [[7, 9]]
    assert abs(-1.3 / ((5 + 1 + 1) / 6.0) - -1.1142857142857143) < 1e-15
    # an all-EOS frame ends the search: what follows it is never looked at
    assert D.backtrace([[[-1.0, -2.0]], [[-0.1, -0.2]]], [[[2, 2]], [[5, 6]]], ptrs, 2, 0, 4) == [[2, 0, 0, 0]]
    # strict >: of two equal candidates the first one found stays
    assert D.backtrace([[[-1.0, -1.0]]], [[[5, 6]]], [[[0, 0]]], 2, 0) == [[5]]


def test_length_penalty_on_the_tiny_traces(D):
    g = gold("tiny")
    T, eos = int(g["steps"]), int(g["eos_token_id"])
    sc = [g["total_scores_%d" % t].tolist() for t in range(T)]
    ids = [g["step_ids_%d" % t].tolist() for t in range(T)]
    ptr = [g["back_ptrs_%d" % t].tolist() for t in range(T)]
    got = D.backtrace(sc, ids, ptr, eos, 1.0)
    for b in range(len(got)):
        # worked out here: every EOS-ended or last-frame candidate, its score over (5 + fid + 1) / 6, first strict maximum
        last = next((t for t in range(T) if all(w == eos for w in ids[t][b])), T - 1)
        cands = [(sc[t][b][k] / ((5 + t + 1) / 6.0), t, k) for t in range(last + 1) for k in range(len(ids[t][b])) if ids[t][b][k] == eos or t == last]
        best = max(c[0] for c in cands)
        _, t, k = next(c for c in cands if c[0] == best)
        seq = [ids[t][b][k]]
        while t > 0:
            k = ptr[t][b][k]
            t -= 1
            seq.append(ids[t][b][k])
        assert got[b] == seq[::-1], b


def test_ngram_ban_rule_on_hand_made_sequences(D):
    assert D.banned_tokens([5, 6], 3) == []                                   # shorter than n
    assert D.banned_tokens([], 3) == [] and D.banned_tokens([5, 6, 7], 4) == []
    assert D.banned_tokens([5, 6, 7, 5, 6], 3) == [7]                         # one repeat
    assert D.banned_tokens([5, 6, 7, 5, 6, 8, 5, 6], 3) == [7, 8]             # two different continuations
    assert D.banned_tokens([4, 4, 4], 3) == [4]                               # the tail overlapping itself: a a a
    assert D.banned_tokens([4, 4], 3) == [] and D.banned_tokens([9, 4, 4], 3) == []
    assert D.banned_tokens([5, 6, 7], 3) == []                                # the tail itself is not a repeat
    assert D.banned_tokens([5, 6, 5], 2) == [6] and D.banned_tokens([5, 6, 5], 1) == [5, 6]
    g_ = torch.Generator().manual_seed(1)
    z = torch.randn(3, 16, generator=g_)
    seqs = [[5, 6, 7, 5, 6], [4, 4, 4], [1, 2]]
    got = D.log_scores_reference(z, seqs, 3, eos_id=4, forbid_eos=False)
    want = torch.log_softmax(z.double(), -1)
    want[0, 7] += -10000.0
    want[1, 4] += -10000.0
    assert got.dtype == torch.float64 and torch.equal(got, want)
    got = D.log_scores_reference(z, seqs, 3, eos_id=4, forbid_eos=True)       # the n-gram penalty is ADDED, the EOS one SET
    want[:, 4] = -10000.0
    assert torch.equal(got, want) and float(got[1, 4]) == -10000.0 and float(got[0, 7]) < -10000.0


def test_merge_ties_take_the_lowest_candidate(D):
    vals = torch.tensor([[-1.0, -2.0], [-1.0, -2.0]])
    ids = torch.tensor([[3, 4], [5, 6]], dtype=torch.int32)
    k_scores, k_ids, back, merged = D.merge_beams(vals, ids, torch.tensor([[-0.5, -0.5]]), torch.zeros(1, 2), 2)
    assert k_ids.tolist() == [[3, 5]] and back.tolist() == [[0, 1]] and k_scores.tolist() == [[-1.5, -1.5]]
    # a beam that ended carries -10000: its continuations lose to every live one
    k_scores, k_ids, back, _ = D.merge_beams(vals, ids, torch.tensor([[-0.5, -0.5]]), torch.tensor([[1.0, 0.0]]), 2)
    assert back.tolist() == [[1, 1]] and k_ids.tolist() == [[5, 6]]


def test_size_rule_and_refusals(D, tmp_path):
    # the reference's length = input_ids.size(0) + max_length: the batch size, so steps = bsz + max_length - len(prompt_ids)
    for bsz, plen, max_length in ((3, 3, 6), (2, 3, 6), (16, 1, 20), (1, 4, 20)):
        length, steps = D.generation_lengths(bsz, plen, max_length, 512)
        assert length == bsz + max_length and steps == bsz + max_length - plen
    for name in ("tiny", "base_shallow"):
        g = gold(name)
        assert int(g["steps"]) == D.generation_lengths(g["output_ids"].shape[0], len(g["prompt_ids"]), int(g["max_length"]), 512)[1]
        assert g["output_ids"].shape[1] == g["output_ids"].shape[0] + int(g["max_length"])
    with pytest.raises(ValueError, match="max_position_embeddings"):
        D.generation_lengths(48, 3, 20, 64)                                   # 68 positions, a table of 64
    with pytest.raises(ValueError, match="Lmax"):
        D.generation_lengths(120, 3, 20, 512)
    with pytest.raises(ValueError, match="prompt"):
        D.generation_lengths(2, 16, 20, 512)
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    cfg = model_config("tiny", str(tmp_path))
    cfg.update(label_smoothing=0.1, prompt="", cls_token_id=1)
    model = mg.XVLMForMLMCaptioning(cfg)                                      # no vocab.txt: the fallback tokenizer namespace
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generation_token_ids()
    model = mg.XVLMForMLMCaptioning(dict(cfg, eos_token_id=2))
    with pytest.raises(ValueError, match="mask_token_id"):
        model.generation_token_ids()
    model = mg.XVLMForMLMCaptioning(dict(cfg, eos_token_id=2, mask_token_id=3))
    assert model.generation_token_ids() == (2, 3)
    # the argument is checked first: no image tensor on the HIP device -> the host path that does not exist
    for call in (lambda: model.generate(None), lambda: model.generate(torch.zeros(1, 3, 32, 32)),
                 lambda: model.beam_search(torch.zeros(1, 3, 32, 32), None, None, None, None)):
        with pytest.raises(NotImplementedError, match="follow-up"):
            call()
    assert model.training                                                      # nothing was touched


def test_decode_entry_points_check_arguments_without_launching():
    h = importlib.import_module("x2-vlm_amd._lib").lib()
    one = ctypes.c_void_p(16)                 # any aligned non-null address: every check below returns before anything is dereferenced
    cases = [(lambda: h.x2_attn_decode(None, 384, one, one, 128, 1, 2, 1, 0, 128, 0.125, None), b"null"),
             (lambda: h.x2_attn_decode(one, 384, one, one, 128, 1, 2, 17, 0, 128, 0.125, None), b"n_new"),
             (lambda: h.x2_attn_decode(one, 384, one, one, 128, 1, 2, 2, 127, 128, 0.125, None), b"exceeds Lmax"),
             (lambda: h.x2_attn_decode(one, 384, one, one, 128, 1, 2, 1, 0, 136, 0.125, None), b"Lmax"),
             (lambda: h.x2_attn_decode(one, 384, one, one, 128, 1, 2, 1, 0, 36, 0.125, None), b"multiple of 8"),
             (lambda: h.x2_attn_decode(one, 380, one, one, 128, 1, 2, 1, 0, 128, 0.125, None), b"qkv_ld"),
             (lambda: h.x2_beam_gather(one, one, one, 2, 3, 128, 256, 5, None), b"src == dst"),
             (lambda: h.x2_beam_gather(one, ctypes.c_void_p(16 + 4096), one, 2, 3, 128, 256, 5, None), b"overlapping"),
             (lambda: h.x2_beam_gather(one, ctypes.c_void_p(1 << 30), one, 2, 3, 128, 256, 0, None), b"hist"),
             (lambda: h.x2_beam_gather(one, ctypes.c_void_p(1 << 30), one, 2, 3, 128, 256, 129, None), b"hist"),
             (lambda: h.x2_logprob_topk(one, 64, 64, 2, None, 0, 0, 0, 0, 0, 9, one, one, None, None), b"K=9"),
             (lambda: h.x2_logprob_topk(one, 60, 64, 2, None, 0, 0, 0, 0, 0, 3, one, one, None, None), b"ldv"),
             (lambda: h.x2_logprob_topk(one, 64, 64, 2, None, 0, 0, 0, 64, 0, 3, one, one, None, None), b"eos_id"),
             (lambda: h.x2_logprob_topk(one, 64, 64, 2, one, 4, 5, 3, 0, 0, 3, one, one, None, None), b"seq_len")]
    for call, word in cases:
        assert call() == -1 and word in h.x2_last_error(), (word, h.x2_last_error())
