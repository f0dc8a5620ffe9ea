#!/usr/bin/env python3
"""VQA fine-tune train step (XVLMForVQA.forward(train=True) + backward, train mode) and its LM head alone.  GPU box only.  Geometry: X2VLM-base -
BEiT2-base 384 px (N = 577), BERT-base 12 + 6 layers, a 6-layer answer decoder, V = 30522 - at batch 8, the per-GPU batch of
configs/finetune/vqa2_base.yaml (that file trains at 768 px), 30-token questions, three answers per question of La = 8, synthetic weights.
Two parts, each a fresh child process under its own `timeout` (the parent never opens the GPU; a part that fails ends the run):
  head    ms per forward + backward of the LM head alone on the S * (La - 1) = 168 scored rows [168, 768] -> the weighted per-answer loss:
          engine.SeqLmLossFn (logits never stored) against the transform followed by materialised fp32 logits, F.cross_entropy(reduction='none'),
          the per-answer sums and the weighted sum in ATen on the same rows.  The two forms alternate in four rounds; eager launches, so host
          time is part of what is compared
  step    ms per step (median of HIP-event intervals of 10 steps after 3 warm-up steps, with min and max), launched eagerly and as one
          graph.GraphedStep replay, k a device tensor
Prints one JSON line per part.  Nothing is asserted on the times.  The optimizer step is not timed.
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ANSWERS = 3
ROUNDS = 4
LIMITS = {"head": 240, "step": 420}          # seconds per part


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
                text_num_hidden_layers=18, text_fusion_start_at=12, embed_dim=256, temp=0.07, max_tokens=40, pad_token_id=0, num_dec_layers=6)


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


def part_head(args):
    import torch
    import torch.nn.functional as F
    engine = importlib.import_module("x2-vlm_amd.engine")
    xbert = importlib.import_module("x2-vlm_amd.xbert")
    K = importlib.import_module("x2-vlm_amd.kernels")
    dev = torch.device("cuda:0")
    cfg = xbert.BertConfig(num_hidden_layers=1)
    cfg.fusion_layer, cfg.encoder_width = 0, 768
    dec = xbert.BertLMHeadModel(cfg).to(dev)
    S, T, V = args.batch * ANSWERS, args.answer_len - 1, cfg.vocab_size
    g = torch.Generator().manual_seed(5)
    rows = torch.randn(S * T, 768, generator=g).to(dev).requires_grad_()
    labels = torch.randint(1000, V, (S, T), generator=g)
    labels[torch.rand(S, T, generator=g) < 0.3] = -100
    labels = labels.reshape(-1).to(dev)
    c = (torch.randint(1, 11, (S,), generator=g).float() / 10.0 / args.batch).to(dev)
    pr = dec.cls.predictions
    head = (cfg.layer_norm_eps, pr.transform.dense.weight, pr.transform.dense.bias, pr.transform.LayerNorm.weight, pr.transform.LayerNorm.bias,
            pr.bias, dec.bert.embeddings.word_embeddings.weight)
    params = [p for p in head[1:]]
    seen = {}

    def clear():
        rows.grad = None
        for p in params:
            p.grad = None

    def fused():
        clear()
        _, total = engine.SeqLmLossFn.apply(rows, labels, T, c, *head)
        total.backward()
        seen["fused"] = total.detach()

    def materialised():
        clear()
        t = F.layer_norm(F.gelu(F.linear(rows, pr.transform.dense.weight, pr.transform.dense.bias)), (768,), pr.transform.LayerNorm.weight,
                         pr.transform.LayerNorm.bias, cfg.layer_norm_eps)
        logits = F.linear(t, dec.bert.embeddings.word_embeddings.weight, pr.bias)
        total = (c * F.cross_entropy(logits, labels, ignore_index=-100, reduction="none").view(S, T).sum(1)).sum()
        total.backward()
        seen["materialised"] = total.detach()

    forms = [("materialised", materialised), ("fused", fused)]
    ms = {name: [] for name, _ in forms}
    for _ in range(ROUNDS):                                       # the forms alternate, so that a busy host meets both
        for name, fn in forms:
            ms[name] += intervals(torch, fn, args.head_steps // ROUNDS, 10)
    out = {}
    for name, v in ms.items():
        med, lo, hi = summary(v)
        out["head_%s_ms" % name] = round(med, 4)
        out["head_%s_ms_min_max" % name] = [round(lo, 4), round(hi, 4)]
    out["head_loss"] = {k: round(float(v), 5) for k, v in seen.items()}
    assert K.round_up(V, 64) == 30528
    print(json.dumps(dict({"probe": "vqa train LM head (fwd+bwd)", "rows": S * T, "hidden": 768, "vocab": V, "head_steps": args.head_steps}, **out)))


def part_step(args):
    import torch
    from types import SimpleNamespace
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    graph = importlib.import_module("x2-vlm_amd.graph")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        model = mg.XVLMForVQA(write_configs(d))
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).train()
    B = args.batch
    b = synthetic.synth_vqa_train_batch(1, B, 30, 384, 30522, [ANSWERS] * B, args.answer_len)
    b = {k: v.to(dev) for k, v in b.items()}
    q = SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"])
    a = SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"])
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        loss = model(b["image"], q, a, k=b["k"], weights=b["weights"], train=True)
        loss.backward()
        return loss

    out = {}
    med, lo, hi = summary(intervals(torch, step, args.steps, args.warmup))
    out.update(eager_ms_per_step=round(med, 2), eager_ms_min_max=[round(lo, 2), round(hi, 2)])
    gstep = graph.GraphedStep(step)
    out["graph_mode"] = gstep.mode
    med, lo, hi = summary(intervals(torch, gstep, args.steps, args.warmup))
    out.update(graphed_ms_per_step=round(med, 2), graphed_ms_min_max=[round(lo, 2), round(hi, 2)], questions_per_s=round(B * 1000.0 / med, 1))
    loss = gstep()
    print(json.dumps(dict({"probe": "vqa train step (fwd+bwd)", "geometry": "BEiT2-base 384px + BERT-base 12+6 layers + 6-layer decoder, V = 30522, "
                           "batch %d, %d answers per question of %d tokens, 30-token questions, train mode" % (B, ANSWERS, args.answer_len),
                           "steps": args.steps, "warmup": args.warmup, "loss": round(float(loss.detach()), 5)}, **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--answer-len", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--head-steps", type=int, default=200)
    ap.add_argument("--part", choices=["head", "step"], help="run this part in this process (what the parent starts under `timeout`)")
    args = ap.parse_args()
    if args.part:
        {"head": part_head, "step": part_step}[args.part](args)
        return
    for part in ("head", "step"):
        cmd = ["timeout", "-k", "10", str(LIMITS[part]), sys.executable, os.path.abspath(__file__), "--part", part] + sys.argv[1:]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            raise SystemExit("bench_vqa_train: part %s ended with status %d; nothing more is started" % (part, rc))


if __name__ == "__main__":
    main()
