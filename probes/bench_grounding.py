#!/usr/bin/env python3
"""Grounding fine-tune train step (XVLMForGrounding forward + backward, train mode) at the RefCOCO+ geometry of the reference's
configs/finetune/refcoco_grounding_large.yaml: BEiT2-large 384 px (N = 577), BERT-large 12 + 6 layers, batch 20, 40 tokens.  Prints one
JSON line with
  eager / graphed   ms per step (median of HIP-event intervals), launched eagerly and as one graph.GraphedStep replay
  box tail          ms per forward + backward of the box tail alone on [batch, 4] logits: XVLMBase.get_bbox_loss on sigmoid(logits) (the
                    ATen chain, the baseline) against ops.bbox_loss (two launches); eager launches, so host time is what is compared
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


def timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for i in range(steps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(steps))
    return ms[len(ms) // 2], ms[0], ms[-1]


def bench(args):
    import numpy as np
    import torch
    mgr = importlib.import_module("x2-vlm_amd.model_grounding")
    graph = importlib.import_module("x2-vlm_amd.graph")
    ops = importlib.import_module("x2-vlm_amd.ops")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        model = mgr.XVLMForGrounding(write_configs(d))
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).train()
    b = synthetic.synth_batch(1, args.batch, 40, 384, 30522, ragged=True)
    r = np.random.default_rng(2)
    wh = r.uniform(0.15, 0.6, size=(args.batch, 2))
    target = torch.from_numpy(np.concatenate([r.uniform(0, 1, size=(args.batch, 2)) * (1 - wh) + wh / 2, wh], 1).astype(np.float32)).to(dev)
    image, ids, atts = b["image"].to(dev), b["text_ids"].to(dev), b["text_atts"].to(dev)
    params = list(model.parameters())
    out = {}

    def step():
        for p in params:
            p.grad = None
        _, loss_bbox, loss_giou = model(image, ids, atts, target)
        (loss_bbox + loss_giou).backward()
        return loss_bbox, loss_giou

    # the box tail alone: the same logits through both forms
    logits = torch.randn(args.batch, 4, device=dev, requires_grad=True)

    def tail_aten():
        logits.grad = None
        lb, lg = model.get_bbox_loss(logits.sigmoid(), target)
        (lb + lg).backward()

    def tail_hip():
        logits.grad = None
        _, lb, lg = ops.bbox_loss(logits, target)
        (lb + lg).backward()

    for name, fn in (("aten", tail_aten), ("hip", tail_hip)):
        med, lo, hi = timed(torch, fn, args.tail_steps, 10)
        out["box_tail_%s_ms" % name] = round(med, 4)
        out["box_tail_%s_ms_min_max" % name] = [round(lo, 4), round(hi, 4)]
    med, lo, hi = timed(torch, step, args.steps, args.warmup)
    out.update(eager_ms_per_step=round(med, 2), eager_ms_min_max=[round(lo, 2), round(hi, 2)])
    gstep = graph.GraphedStep(step)
    out["graph_mode"] = gstep.mode
    med, lo, hi = timed(torch, gstep, args.steps, args.warmup)
    out.update(graphed_ms_per_step=round(med, 2), graphed_ms_min_max=[round(lo, 2), round(hi, 2)], pairs_per_s=round(args.batch * 1000.0 / med, 1))
    lb, lg = gstep()
    print(json.dumps(dict({"probe": "grounding train step (fwd+bwd)", "geometry": "BEiT2-large 384px + BERT-large 12+6 layers, batch %d, 40 tokens, "
                           "train mode" % args.batch, "steps": args.steps, "warmup": args.warmup, "loss_bbox": round(float(lb), 5),
                           "loss_giou": round(float(lg), 5)}, **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tail-steps", type=int, default=200)
    bench(ap.parse_args())


if __name__ == "__main__":
    main()
