#!/usr/bin/env python3
"""Captioning fine-tune train step (XVLMForMLMCaptioning forward + backward, train mode) at the shipped geometry of
configs/finetune/coco_captioning_large.yaml: BEiT2-large 384 px (N = 577), BERT-large 18 layers (fusion from 12), batch 16, FG-free collate
with max_tokens 40 + max_masks 18 (L = 58), V = 30522.  Prints one JSON line: ms per step (median of HIP-event intervals) and
image-caption pairs/s.  The optimizer step is not timed.

Kernel shares: run under the profiler and summarise its kernel statistics table:
  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o cap -- python probes/bench_captioning.py --steps 5 --warmup 2
  python probes/bench_captioning.py --summarize OUT/.../cap_kernel_stats.csv
"""
import argparse
import csv
import importlib
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# the kernels the captioning path adds (demangled names as the profiler prints them)
NEW = [("attention, 2-D mask (fwd / dQ / dK-dV)", re.compile(r"^(void )?attn_(fwd|bwd_dq|bwd_dkv)_kernel<.*true>")),
       ("fused MLM head, smoothed (variants 11 / 12)", re.compile(r"^(void )?gemm_nt_kernel<\d+, 1[12]")),
       ("smoothed-loss combine / reduce", re.compile(r"^(void )?ls_(combine|reduce)_kernel")),
       ("embedding with position ids", re.compile(r"^(void )?(embed_fwd_pid|embed_rowsum)_kernel")),
       ("2-D additive mask", re.compile(r"^(void )?additive_mask2d_kernel"))]


def write_configs(d):
    vis = os.path.join(d, "config_beit2_large.json")
    with open(vis, "w") as f:
        json.dump({"ckpt": "", "vision_width": 1024, "patch_size": 16}, f)
    tdir = os.path.join(d, "bert-large-uncased-12l")
    os.makedirs(tdir, exist_ok=True)
    with open(os.path.join(tdir, "config.json"), "w") as f:
        json.dump(dict(vocab_size=30522, hidden_size=1024, num_attention_heads=16, intermediate_size=4096, max_position_embeddings=512,
                       type_vocab_size=2, hidden_act="gelu", hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1, layer_norm_eps=1e-12,
                       initializer_range=0.02, pad_token_id=0, model_type="bert"), f)
    return dict(use_beit_v2=True, vision_config=vis, image_res=384, patch_size=16, vision_num_hidden_layers=24, text_encoder=tdir,
                text_num_hidden_layers=18, text_fusion_start_at=12, embed_dim=256, temp=0.07, max_tokens=40, max_masks=18,
                label_smoothing=0.1, prompt="", cls_token_id=101)


def bench(args):
    import torch
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        model = mg.XVLMForMLMCaptioning(write_configs(d))
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).train()
    b = synthetic.synth_captioning_batch(1, args.batch, 40, 18, 384, 30522, fg_free=True)
    b = {k: v.to(dev) for k, v in b.items()}
    inputs = (b["image"], b["text_ids_masked"], b["text_atts"], b["position_ids"], b["masked_pos"], b["masked_ids"], b["masked_weight"])

    def step():
        for p in model.parameters():
            p.grad = None
        loss = model(*inputs)
        loss.backward()
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    ev[0].record()
    for i in range(args.steps):
        loss = step()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
    med = ms[len(ms) // 2]
    print(json.dumps({"probe": "captioning train step (fwd+bwd)", "geometry": "BEiT2-large 384px + BERT-large 18 layers, batch %d, L = 58, "
                      "18 masks, V = 30522, FG-free, train mode" % args.batch, "ms_per_step": round(med, 2),
                      "ms_min_max": [round(ms[0], 2), round(ms[-1], 2)], "pairs_per_s": round(args.batch * 1000.0 / med, 1),
                      "steps": args.steps, "warmup": args.warmup, "loss": round(float(loss), 5)}))


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    out = {}
    for label, rx in NEW:
        ns = sum(float(r["TotalDurationNs"]) for r in rows if rx.search(r["Name"]))
        out[label] = round(100.0 * ns / tot, 2)
    out["all new kernels"] = round(sum(out.values()), 2)
    print(json.dumps({"share_of_kernel_time_percent": out, "total_kernel_ms": round(tot / 1e6, 2)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--summarize", default=None, help="kernel statistics CSV of a rocprofv3 --kernel-trace --stats run of this probe")
    args = ap.parse_args()
    if args.summarize is not None:
        summarize(args.summarize)
    else:
        bench(args)


if __name__ == "__main__":
    main()
