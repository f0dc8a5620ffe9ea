#!/usr/bin/env python3
"""NLVR2 fine-tune train step (XVLMForNLVR forward + backward, train mode).  The reference ships no NLVR yaml, so the geometry is this
project's: BEiT2-large 384 px (N = 577), BERT-large 12 + 6 layers, 10 pairs (20 images), 40 tokens, synthetic weights.  Prints one JSON line with
  eager / graphed   ms per step (median of HIP-event intervals), launched eagerly and as one graph.GraphedStep replay
  cls tail          ms per forward + backward of the head's tail alone - LayerNorm -> GELU -> Linear(H -> 2) -> cross_entropy on fp32 rows [R, H] -
                    at [10, 4096] (this step) and [64, 3072] (X2VLM-base at batch 64): ops.cls_tail (two launches each way) against the ATen
                    chain (F.layer_norm, F.gelu, F.linear, F.cross_entropy).  The project's own unfused chain - ops.layer_norm + ops.gelu +
                    ops.linear + ops.cross_entropy - cannot run there: x2_layernorm_fwd takes rows of at most 2048 columns.  It is timed
                    against ops.cls_tail at [10, 2048] and [64, 2048], the widest rows it takes.  The forms alternate in four rounds; eager
                    launches, so host time is what is compared
Nothing is asserted on the times.  The optimizer step is not timed.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAIL_SHAPES = [(10, 4096), (64, 3072), (10, 2048), (64, 2048)]
UNFUSED_MAX_H = 2048          # x2_layernorm_fwd's widest row
ROUNDS = 4


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
                text_num_hidden_layers=18, text_fusion_start_at=12, embed_dim=256, temp=0.07, max_tokens=40)


def intervals(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) for i in range(steps)]


def summary(ms):
    ms = sorted(ms)
    return ms[len(ms) // 2], ms[0], ms[-1]


def timed(torch, fn, steps, warmup):
    return summary(intervals(torch, fn, steps, warmup))


def bench_tail(torch, ops, xvlm, dev, R, H, steps):
    """forward + backward of the tail on the same rows through every form -> {name: (median, min, max)}, {name: loss}"""
    import torch.nn.functional as F
    head = xvlm.build_mlp(H // 2, 2).to(dev)                      # seq[1]: LayerNorm(H), seq[3]: Linear(H -> 2)
    h = torch.randn(R, H, device=dev, requires_grad=True)
    targets = (torch.arange(R, device=dev) % 2).long()
    tail = [head[1].weight, head[1].bias, head[3].weight, head[3].bias]
    seen = {}

    def clear():
        h.grad = None
        for p in tail:
            p.grad = None

    def unfused():
        clear()
        y = ops.gelu(ops.layer_norm(h, head[1].weight, head[1].bias, head[1].eps))
        loss = ops.cross_entropy(ops.linear(y, head[3].weight, head[3].bias), targets)
        loss.backward()
        seen["unfused"] = loss.detach()

    def aten():
        clear()
        y = F.gelu(F.layer_norm(h, (H,), head[1].weight, head[1].bias, head[1].eps))
        loss = F.cross_entropy(F.linear(y, head[3].weight, head[3].bias), targets, ignore_index=-100)
        loss.backward()
        seen["aten"] = loss.detach()

    def fused():
        clear()
        _, loss = ops.cls_tail(head, h, targets)
        loss.backward()
        seen["fused"] = loss.detach()

    forms = [("aten", aten), ("fused", fused)] + ([("unfused", unfused)] if H <= UNFUSED_MAX_H else [])
    ms = {name: [] for name, _ in forms}
    for _ in range(ROUNDS):                                       # the forms alternate, so that a busy host meets all of them
        for name, fn in forms:
            ms[name] += intervals(torch, fn, steps // ROUNDS, 10)
    return {k: summary(v) for k, v in ms.items()}, {k: round(float(v), 6) for k, v in seen.items()}


def bench(args):
    import torch
    mcl = importlib.import_module("x2-vlm_amd.model_classification")
    graph = importlib.import_module("x2-vlm_amd.graph")
    ops = importlib.import_module("x2-vlm_amd.ops")
    xvlm = importlib.import_module("x2-vlm_amd.xvlm")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    out = {}
    for R, H in TAIL_SHAPES:
        t, losses = bench_tail(torch, ops, xvlm, dev, R, H, args.tail_steps)
        for name, (med, lo, hi) in t.items():
            out["cls_tail_%s_ms_%dx%d" % (name, R, H)] = round(med, 4)
            out["cls_tail_%s_ms_min_max_%dx%d" % (name, R, H)] = [round(lo, 4), round(hi, 4)]
        out["cls_tail_loss_%dx%d" % (R, H)] = losses
    if args.tail_only:
        print(json.dumps(dict({"probe": "nlvr cls tail (fwd+bwd)", "tail_steps": args.tail_steps}, **out)))
        return
    with tempfile.TemporaryDirectory() as d:
        model = mcl.XVLMForNLVR(write_configs(d))
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).train()
    b = synthetic.synth_batch(1, 2 * args.pairs, 40, 384, 30522, ragged=True)
    image, ids, atts = b["image"].to(dev), b["text_ids"][:args.pairs].to(dev), b["text_atts"][:args.pairs].to(dev)
    targets = (torch.arange(args.pairs, device=dev) % 2).long()
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        loss = model(image, ids, atts, targets, train=True)
        loss.backward()
        return loss

    med, lo, hi = timed(torch, step, args.steps, args.warmup)
    out.update(eager_ms_per_step=round(med, 2), eager_ms_min_max=[round(lo, 2), round(hi, 2)])
    gstep = graph.GraphedStep(step)
    out["graph_mode"] = gstep.mode
    med, lo, hi = timed(torch, gstep, args.steps, args.warmup)
    out.update(graphed_ms_per_step=round(med, 2), graphed_ms_min_max=[round(lo, 2), round(hi, 2)], pairs_per_s=round(args.pairs * 1000.0 / med, 1))
    loss = gstep()
    print(json.dumps(dict({"probe": "nlvr train step (fwd+bwd)", "geometry": "BEiT2-large 384px + BERT-large 12+6 layers, %d pairs (%d images), "
                           "40 tokens, train mode" % (args.pairs, 2 * args.pairs), "steps": args.steps, "warmup": args.warmup,
                           "loss": round(float(loss), 5)}, **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tail-steps", type=int, default=200)
    ap.add_argument("--tail-only", action="store_true")
    bench(ap.parse_args())


if __name__ == "__main__":
    main()
