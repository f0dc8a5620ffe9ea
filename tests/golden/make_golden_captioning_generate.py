#!/usr/bin/env python3
"""Golden vectors for captioning inference: the REAL reference model's generate() / beam_search (models/model_generation.py:113-397) on CPU
fp32, seeded synthetic weights, the image of the case's seeded captioning batch (plain collate form).  As make_golden_captioning.py, plus: the tokenizer gets
the two special tokens the reference's build_tokenizer adds (bos = [CLS], eos = [SEP]), and torch.Tensor.cuda is an identity for the run
(the reference calls .cuda() on its n-gram mask).  Build container only.

Recorded per case by wrapping torch.topk and hooking text_encoder.cls, per step t (step 0 has B rows, later steps B * K):
  output_ids                       what generate()'s beam_search returned (padded pred_seq lists)
  step_ids_t, back_ptrs_t, total_scores_t        [B, K] selections of the step
  logs_t                           [S, V] log-scores as handed to the first topk (penalties applied), V <= 1024 only
  top_vals_t, top_ids_t            [S, 16] largest log-scores and their columns (every case)
  lse_t [S], maxabs_t []           logsumexp and max-abs of the step's raw logits
  margin1_t [S], margin2_t [B]     K-th minus (K+1)-th value of the per-row topk and of the [B, K * K] merge topk (inf at step 0)

writes tests/golden/<case>_captioning_generate.npz for GEN_CASES
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
import reference_shims  # noqa: E402
from cases import CASES  # noqa: E402
from cases_captioning import CAP_CASES, caption_config, write_vocab  # noqa: E402

synthetic = importlib.import_module("x2-vlm_amd.synthetic")

PROMPT = "w7 w9"
GEN_CASES = {
    "tiny": dict(num_beams=3, max_length=6, min_length=2),
    "base_shallow": dict(num_beams=3, max_length=6, min_length=2),
}
TOP = 16


def bert_tokenizer(path, *a, **k):
    from transformers import BertTokenizer
    tok = BertTokenizer(os.path.join(path, "vocab.txt"), do_lower_case=True)
    tok.add_special_tokens({"bos_token": tok.cls_token})         # dataset/tokenizers/__init__.py: "always use cls and sep"
    tok.add_special_tokens({"eos_token": tok.sep_token})
    return tok


def run_case(name):
    cc = CAP_CASES[name]
    c = CASES[cc["case"]]
    gen = GEN_CASES[name]
    K = gen["num_beams"]
    workdir = "/tmp/x2golden_capgen_%s" % name
    cfg = caption_config(cc["case"], workdir)
    cfg["prompt"] = PROMPT
    write_vocab(cfg["text_encoder"], c["vocab"])
    from models.model_generation import XVLMForMLMCaptioning
    model = XVLMForMLMCaptioning(config=cfg)
    tok = model.tokenizer
    assert tok.vocab_size == c["vocab"] and tok.eos_token_id == tok.sep_token_id
    assert model.prompt_ids == [tok.cls_token_id, 7, 9], model.prompt_ids
    synthetic.synth_state_dict(model, cc["wseed"])
    model.eval()
    image = synthetic.synth_captioning_batch(cc["bseed"], cc["batch"], cc["max_tokens"], cc["max_masks"], c["image_res"], c["vocab"], fg_free=False)["image"]
    B = image.shape[0]

    topk_calls, logits = [], []
    real_topk, real_cuda = torch.topk, torch.Tensor.cuda

    def topk(x, k, *a, **kw):
        topk_calls.append(x.detach().clone())
        return real_topk(x, k, *a, **kw)
    hook = model.text_encoder.cls.register_forward_hook(lambda m, i, o: logits.append(o.detach().clone()))
    torch.topk, torch.Tensor.cuda = topk, lambda self, *a, **k: self
    try:
        with torch.no_grad():
            captions = model.generate(image, **gen)
            topk_calls_gen, logits_gen = list(topk_calls), list(logits)
            # the same call once more through beam_search for the id lists generate() decodes (deterministic: eval, no sampling)
            del topk_calls[:], logits[:]
            length = B + gen["max_length"]
            ids = torch.tensor(model.prompt_ids).view(1, -1).expand(B, -1)
            output_ids = model.beam_search(image, ids, torch.zeros(B, length, dtype=torch.long), torch.arange(length).view(1, -1).expand(B, -1),
                                           torch.tril(torch.ones(length, length, dtype=torch.long)).view(1, length, length).expand(B, length, length),
                                           num_beams=K, min_length=gen["min_length"])
    finally:
        torch.topk, torch.Tensor.cuda = real_topk, real_cuda
        hook.remove()
    assert len(topk_calls) == len(topk_calls_gen) and all(torch.equal(a, b) for a, b in zip(topk_calls, topk_calls_gen))
    steps = len(logits)
    assert steps == B + gen["max_length"] - len(model.prompt_ids) and len(topk_calls) == 2 * steps - 1
    out = dict(output_ids=np.array(output_ids, dtype=np.int64), prompt_ids=np.array(model.prompt_ids), eos_token_id=np.array(tok.eos_token_id),
               mask_token_id=np.array(tok.mask_token_id), num_beams=np.array(K), max_length=np.array(gen["max_length"]),
               min_length=np.array(gen["min_length"]), steps=np.array(steps), captions=np.array(captions))
    prev_scores = prev_eos = None
    ci = 0
    for t in range(steps):
        ls = topk_calls[ci].reshape(-1, c["vocab"])
        ci += 1
        S = ls.shape[0]
        assert S == (B if t == 0 else B * K)
        v, i = real_topk(ls, max(TOP, K + 1))
        out["top_vals_%d" % t], out["top_ids_%d" % t] = v[:, :TOP].numpy(), i[:, :TOP].numpy()
        out["margin1_%d" % t] = (v[:, K - 1] - v[:, K]).numpy()
        if c["vocab"] <= 1024:
            out["logs_%d" % t] = ls.numpy()
        z = logits[t].reshape(S, -1).double()
        out["lse_%d" % t] = torch.logsumexp(z, -1).numpy()
        out["maxabs_%d" % t] = np.array(float(z.abs().max()))
        if t == 0:
            k_scores, k_ids = v[:, :K], i[:, :K]
            back = torch.zeros(B, K, dtype=torch.long)
            out["margin2_%d" % t] = np.full(B, np.inf, dtype=np.float32)
        else:
            kk = topk_calls[ci]
            ci += 1
            assert kk.shape == (B, K * K)
            # the recorded merge input must be what the merge rule gives from the recorded row scores
            want = (v[:, :K] + (prev_eos * -10000.0 + prev_scores).reshape(B * K, 1)).reshape(B, K * K)
            assert torch.equal(want, kk)
            mv, mi = real_topk(kk, K + 1)
            k_scores, back = mv[:, :K], torch.div(mi[:, :K], K, rounding_mode="floor")
            k_ids = torch.gather(i[:, :K].reshape(B, K * K), 1, mi[:, :K])
            out["margin2_%d" % t] = (mv[:, K - 1] - mv[:, K]).numpy()
        out["step_ids_%d" % t], out["back_ptrs_%d" % t], out["total_scores_%d" % t] = k_ids.numpy(), back.numpy(), k_scores.numpy()
        prev_scores, prev_eos = k_scores, (k_ids == tok.eos_token_id).to(k_scores.dtype)
    if name == "tiny":
        assert output_ids[2][:3] == [199, 93, 2] and not any(output_ids[2][3:]), output_ids[2]
    path = os.path.join(HERE, "%s_captioning_generate.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20
    print("wrote", path, os.path.getsize(path), "bytes; output_ids", output_ids, "captions", captions)
    print("  min margins per step:", [(round(float(out["margin1_%d" % t].min()), 5), round(float(out["margin2_%d" % t].min()), 5)) for t in range(steps)])


def main():
    reference_shims.install()
    sys.modules["dataset"].build_tokenizer = bert_tokenizer      # transformers' BertTokenizer on the vocab.txt written above
    reference_shims.ensure_process_group()
    torch.set_num_threads(8)
    for name in (sys.argv[1:] or list(GEN_CASES)):
        run_case(name)


if __name__ == "__main__":
    main()
