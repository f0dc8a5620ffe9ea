#!/usr/bin/env python3
"""VQA answer ranking (XVLMForVQA.forward(train=False)) at the VQA test geometry: X2VLM-base, BEiT2-base 384 px (N = 577), BERT-base 12 + 6
layers, a 6-layer answer decoder, V = 30522; 32 questions of 30 tokens, an answer list of Na = 3128 rows of La = 8 tokens, k = 128 -
S = 4096 candidate rows, 28672 scored positions.  Synthetic weights and batch.  Prints one JSON line:
  ms per call on the fused path (median and range of --calls calls after warm-up) and questions/s,
  the same call with _fused=False (the [S * (La - 1), V] logits materialised, candidate bookkeeping in torch): the baseline,
  and for both, from a SEPARATE call instrumented with HIP events, the split between the vision tower, the question pass, the candidate
  pass (the decoder over S rows), the head on the scored rows and the rest (first step, selection, candidate tensors, re-ranking).
Nothing is gated on these times.  GPU box only."""
import argparse
import importlib
import json
import os
import sys
import tempfile
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_configs(d):
    vis = os.path.join(d, "config_beit2_base.json")
    with open(vis, "w") as f:
        json.dump({"ckpt": "", "vision_width": 768, "patch_size": 16}, f)
    tdir = os.path.join(d, "bert-base-uncased")
    os.makedirs(tdir, exist_ok=True)
    with open(os.path.join(tdir, "config.json"), "w") as f:
        json.dump(dict(vocab_size=30522, hidden_size=768, num_attention_heads=12, intermediate_size=3072, max_position_embeddings=512,
                       type_vocab_size=2, hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12,
                       initializer_range=0.02, pad_token_id=0, model_type="bert"), f)
    return dict(use_beit_v2=True, vision_config=vis, image_res=384, patch_size=16, vision_num_hidden_layers=12, text_encoder=tdir,
                text_num_hidden_layers=18, text_fusion_start_at=12, embed_dim=256, temp=0.07, pad_token_id=0, num_dec_layers=6)


def timed_calls(torch, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms, out


def profile_split(torch, model, S, fn):
    """One call with event pairs around the vision tower, the question pass, the decoder's candidate pass and the head on the scored rows."""
    spans = {"vision": [], "question_pass": [], "candidate_pass": [], "head": []}

    def wrap(f, key, when=lambda *a, **k: True):
        def g(*a, **k):
            if not when(*a, **k):
                return f(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(*a, **k)
            e1.record()
            spans[key].append((e0, e1))
            return r
        return g
    dec = model.text_decoder
    many = lambda rows, *a, **k: rows.shape[0] > S          # noqa: E731  the scored rows, not the first step's B rows
    patched = {(model, "get_vision_embeds"): wrap(model.get_vision_embeds, "vision"),
               (model.text_encoder, "forward"): wrap(model.text_encoder.forward, "question_pass"),
               (dec, "forward"): wrap(dec.forward, "candidate_pass", lambda ids, *a, **k: ids.shape[0] == S),
               (dec, "head_logits"): wrap(dec.head_logits, "head", many), (dec, "head_loss_rows"): wrap(dec.head_loss_rows, "head", many)}
    for (obj, name), g in patched.items():
        setattr(obj, name, g)
    try:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
    finally:
        for obj, name in patched:
            delattr(obj, name)
    out = {k: round(sum(x.elapsed_time(y) for x, y in v), 2) for k, v in spans.items()}
    total = a.elapsed_time(b)
    out["rest"] = round(total - sum(out.values()), 2)
    out["call"] = round(total, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--questions", type=int, default=32)
    ap.add_argument("--answers", type=int, default=3128)
    ap.add_argument("--answer-len", type=int, default=8)
    ap.add_argument("--k", type=int, default=128)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-calls", type=int, default=10, help="timed calls with _fused=False (0: skip the baseline)")
    args = ap.parse_args()
    import torch
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        model = mg.XVLMForVQA(write_configs(d))
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).eval()
    b = {k: v.to(dev) for k, v in synthetic.synth_vqa_batch(1, args.questions, 30, 384, 30522, args.answers, args.answer_len).items()}
    q = SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"])
    a = SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"])
    S = args.questions * args.k

    def call(fused=True):
        return model(b["image"], q, a, k=args.k, train=False, _fused=fused)
    ms, out = timed_calls(torch, call, args.calls, args.warmup)
    med = ms[len(ms) // 2]
    res = {"probe": "VQA answer ranking (forward(train=False))",
           "geometry": "BEiT2-base 384px + BERT-base 12 + 6 layers + 6-layer decoder, %d questions x 30 tokens, Na = %d, La = %d, k = %d, "
                       "S = %d rows, V = 30522" % (args.questions, args.answers, args.answer_len, args.k, S),
           "ms_per_call": round(med, 2), "ms_min_max": [round(ms[0], 2), round(ms[-1], 2)], "questions_per_s": round(args.questions * 1000.0 / med, 1),
           "calls": args.calls, "warmup": args.warmup, "split_ms_profiled_call": profile_split(torch, model, S, call)}
    if args.baseline_calls:
        base, out_b = timed_calls(torch, lambda: call(False), args.baseline_calls, args.warmup)
        bm = base[len(base) // 2]
        res.update(unfused_ms_per_call=round(bm, 2), unfused_ms_min_max=[round(base[0], 2), round(base[-1], 2)], unfused_calls=args.baseline_calls,
                   speedup_over_unfused=round(bm / med, 2), unfused_split_ms_profiled_call=profile_split(torch, model, S, lambda: call(False)),
                   same_best_answers_as_unfused=int((out[0][:, 0] == out_b[0][:, 0]).sum()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
