#!/usr/bin/env python3
"""Captioning inference (XVLMForMLMCaptioning.generate: beam search over cached K/V) at the geometry of probes/bench_captioning.py: BEiT2-large
384 px (N = 577), BERT-large 18 layers (fusion from 12), V = 30522, batch 16, num_beams 3, max_length 20, min_length 5, the prompt
"a picture of" (4 ids with [CLS]) - 16 + 20 - 4 = 32 decode steps on 48 beam rows.  Prints one JSON line:
  ms per generate() call with the cache (median and range of --calls calls after warm-up) and captions/s,
  the same call with the cache bypassed (every step recomputes the whole prefix through the full-sequence forward): the baseline,
  and, from a SEPARATE call instrumented with HIP events (not one of the timed ones), the split between the vision tower, the per-step
  text stack (embedding to MLM-head logits), the scoring kernel and the rest (beam bookkeeping in torch, cache reorder, cross K/V).
GPU box only."""
import argparse
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_captioning import write_configs  # noqa: E402

PROMPT_IDS = [101, 1037, 3861, 1997]          # [CLS] a picture of (bert-base-uncased ids; the bench has no vocab.txt to tokenize with)


def timed_calls(torch, fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()                                   # ends with the search's one device-to-host transfer
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms, out


def profile_split(torch, model, decode, K, fn):
    """One call with event pairs around the vision tower, every text-stack step and every scoring launch."""
    spans = {"vision": [], "text_stack": [], "scoring": []}

    def wrap(f, key):
        def g(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = f(*a, **k)
            e1.record()
            spans[key].append((e0, e1))
            return r
        return g
    saved = (model.get_vision_embeds, decode._TextStack.step, K.logprob_topk)
    model.get_vision_embeds = wrap(saved[0], "vision")
    decode._TextStack.step = wrap(saved[1], "text_stack")
    K.logprob_topk = wrap(saved[2], "scoring")
    try:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
    finally:
        del model.get_vision_embeds
        decode._TextStack.step, K.logprob_topk = saved[1], saved[2]
    out = {k: round(sum(x.elapsed_time(y) for x, y in v), 2) for k, v in spans.items()}
    total = a.elapsed_time(b)
    out["rest"] = round(total - sum(out.values()), 2)
    out["call"] = round(total, 2)
    out["steps"] = len(spans["text_stack"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-calls", type=int, default=3, help="timed calls with the cache bypassed (0: skip the baseline)")
    args = ap.parse_args()
    import torch
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    decode = importlib.import_module("x2-vlm_amd.decode")
    K = importlib.import_module("x2-vlm_amd.kernels")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    gen = dict(num_beams=3, max_length=20, min_length=5)
    with tempfile.TemporaryDirectory() as d:
        model = mg.XVLMForMLMCaptioning(dict(write_configs(d), eos_token_id=102, mask_token_id=103))
    model.prompt_ids = list(PROMPT_IDS)
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).eval()
    image = synthetic.synth_captioning_batch(1, args.batch, 40, 18, 384, 30522, fg_free=False)["image"].to(dev)
    B = args.batch
    length = B + gen["max_length"]
    bs_args = (image, torch.tensor(model.prompt_ids, device=dev).view(1, -1).expand(B, -1), torch.zeros(B, length, dtype=torch.long, device=dev),
               torch.arange(length, device=dev).view(1, -1).expand(B, -1),
               torch.tril(torch.ones(length, length, dtype=torch.long, device=dev)).view(1, length, length).expand(B, length, length))
    bs_kw = dict(num_beams=gen["num_beams"], min_length=gen["min_length"])

    ms, ids = timed_calls(torch, lambda: model.generate(image, **gen), args.calls, args.warmup)
    med = ms[len(ms) // 2]
    res = {"probe": "captioning generate (beam search, cached K/V)",
           "geometry": "BEiT2-large 384px + BERT-large 18 layers, batch %d, %d beams, max_length %d, min_length %d, prompt of %d ids, %d steps, "
                       "V = 30522" % (B, gen["num_beams"], gen["max_length"], gen["min_length"], len(PROMPT_IDS), length - len(PROMPT_IDS)),
           "ms_per_call": round(med, 2), "ms_min_max": [round(ms[0], 2), round(ms[-1], 2)], "captions_per_s": round(B * 1000.0 / med, 1),
           "calls": args.calls, "warmup": args.warmup}
    res["split_ms_profiled_call"] = profile_split(torch, model, decode, K, lambda: model.generate(image, **gen))
    if args.baseline_calls:
        base, ids_b = timed_calls(torch, lambda: model.beam_search(*bs_args, **bs_kw, _use_cache=False), args.baseline_calls, 1)
        bm = base[len(base) // 2]
        res.update(baseline_uncached_ms_per_call=round(bm, 2), baseline_ms_min_max=[round(base[0], 2), round(base[-1], 2)],
                   baseline_calls=args.baseline_calls, speedup_over_uncached=round(bm / med, 2),
                   same_ids_as_uncached=sum(int(a == b) for a, b in zip(ids, ids_b)))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
