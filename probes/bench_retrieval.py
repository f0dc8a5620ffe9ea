#!/usr/bin/env python3
"""Retrieval fine-tune step and evaluation (XVLMForRetrieval with `idx`, csrc/retrieval.hip).  GPU box only, one process.  The reference ships no
retrieval yaml, so the geometry is this project's: BEiT2-large 384 px (N = 577), BERT-large 12 + 6 layers, 40 tokens, synthetic weights, every
image owning one caption pair (ids b // 2).  Prints one JSON line with
  eager / graphed   ms per fine-tune step (forward + backward, train mode, sampled negatives; median of HIP-event intervals), launched eagerly
                    and as one graph.GraphedStep replay
  itc soft          ms per forward + backward of the soft-label ITC loss alone on fp32 logits [N, N], N = 64, 256, 1024: ops.itc_soft (three
                    launches) against the torch chain it replaces (eq, sum, div, two log_softmax, two mul / sum / mean, a transpose, and their
                    autograd).  The forms alternate in four rounds; eager launches, so host time is what is compared
  recall            ms per retrieval_eval of 5 000 x 25 010 random device scores (COCO's 5k test split; five captions per image) against the
                    host route: both matrices copied to the host and every query row sorted in full there
Nothing is asserted on the times.  The optimizer step is not timed.
"""
import argparse
import importlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_nlvr import intervals, summary, timed, write_configs  # noqa: E402

ITC_SIZES = [64, 256, 1024]
ROUNDS = 4


def torch_chain(torch, logits, idx_all):
    """the `idx` branch of get_contrastive_loss as it stood before ops.itc_soft"""
    idx_all = idx_all.view(-1, 1)
    pos = torch.eq(idx_all, idx_all.t()).float()
    lab = pos / pos.sum(1, keepdim=True)
    li = -torch.sum(torch.log_softmax(logits, dim=1) * lab, dim=1).mean()
    lt = -torch.sum(torch.log_softmax(logits.t(), dim=1) * lab, dim=1).mean()
    return (li + lt) / 2


def bench_itc(torch, ops, dev, N, steps):
    g = torch.Generator(device="cpu").manual_seed(N)
    z = (torch.randn(N, N, generator=g) * 4).to(dev).requires_grad_()
    idx = (torch.arange(N, device=dev) // 2).long()
    seen = {}

    def chain():
        z.grad = None
        loss = torch_chain(torch, z, idx)
        loss.backward()
        seen["torch"] = loss.detach()

    def fused():
        z.grad = None
        loss = ops.itc_soft(z, idx)
        loss.backward()
        seen["hip"] = loss.detach()

    ms = {"torch": [], "hip": []}
    for _ in range(ROUNDS):
        for name, fn in (("torch", chain), ("hip", fused)):
            ms[name] += intervals(torch, fn, steps // ROUNDS, 10)
    return {k: summary(v) for k, v in ms.items()}, {k: round(float(v), 6) for k, v in seen.items()}


HOST_ROWS = 256                  # query rows sorted per chunk of the host route


def host_recall_counts(np, scores, gt_offs, gt_ids):
    """The host route for one direction: every query row sorted in full (np.argsort, HOST_ROWS rows at a time), each column's position in that
    order scattered back, and the best position among the row's ground truths (CSR) -> [#best < 1, #best < 5, #best < 10]"""
    R, N = scores.shape
    best = np.full(R, np.iinfo(np.int64).max)
    for r0 in range(0, R, HOST_ROWS):
        order = np.argsort(-scores[r0:r0 + HOST_ROWS], axis=1)
        position = np.empty_like(order)
        np.put_along_axis(position, order, np.arange(N)[None, :], axis=1)
        for k in range(order.shape[0]):
            mine = gt_ids[gt_offs[r0 + k]:gt_offs[r0 + k + 1]]
            if mine.size:
                best[r0 + k] = position[k, mine].min()
    return [int((best < k).sum()) for k in (1, 5, 10)]


def bench_recall(torch, mr, dev, images, captions, repeats):
    import numpy as np
    g = torch.Generator(device="cpu").manual_seed(3)
    i2t = torch.randn(images, captions, generator=g).to(dev)
    t2i = torch.randn(captions, images, generator=g).to(dev)
    per = captions // images
    img2txt = {i: list(range(per * i, per * (i + 1))) for i in range(images)}
    txt2img = [min(j // per, images - 1) for j in range(captions)]
    res = mr.retrieval_eval(i2t, t2i, txt2img, img2txt)              # warm-up
    torch.cuda.synchronize()
    t_dev = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = mr.retrieval_eval(i2t, t2i, txt2img, img2txt)
        t_dev.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    a, b = i2t.cpu().numpy(), t2i.cpu().numpy()
    t_copy = (time.perf_counter() - t0) * 1e3
    counts = []
    for m, gt in ((a, img2txt), (b, txt2img)):
        offs, ids = mr.ground_truth_csr(gt, m.shape[0])
        counts += host_recall_counts(np, m, offs.numpy(), ids.numpy())
    t_host = (time.perf_counter() - t0) * 1e3
    same = [round(res[k] * n / 100.0) for k, n in (("txt_r1", images), ("txt_r5", images), ("txt_r10", images), ("img_r1", captions),
                                                    ("img_r5", captions), ("img_r10", captions))] == counts
    return dict(recall_device_ms=round(sorted(t_dev)[len(t_dev) // 2], 2), recall_device_ms_min_max=[round(min(t_dev), 2), round(max(t_dev), 2)],
                recall_host_ms=round(t_host, 1), recall_host_copy_ms=round(t_copy, 1), recall_counts_equal=same, recall_shape=[images, captions])


def bench(args):
    import torch
    mr = importlib.import_module("x2-vlm_amd.model_retrieval")
    graph = importlib.import_module("x2-vlm_amd.graph")
    ops = importlib.import_module("x2-vlm_amd.ops")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    dev = torch.device("cuda:0")
    out = {}
    for N in ITC_SIZES:
        t, losses = bench_itc(torch, ops, dev, N, args.itc_steps)
        for name, (med, lo, hi) in t.items():
            out["itc_soft_%s_ms_%d" % (name, N)] = round(med, 4)
            out["itc_soft_%s_ms_min_max_%d" % (name, N)] = [round(lo, 4), round(hi, 4)]
        out["itc_soft_loss_%d" % N] = losses
    out.update(bench_recall(torch, mr, dev, args.images, args.captions, args.recall_repeats))
    if args.skip_step:
        print(json.dumps(dict({"probe": "retrieval: itc soft (fwd+bwd), recall", "itc_steps": args.itc_steps}, **out)))
        return
    with tempfile.TemporaryDirectory() as d:
        model = mr.XVLMForRetrieval(write_configs(d))
    synthetic.synth_state_dict(model, 0)
    model = model.to(dev).train()
    b = synthetic.synth_batch(1, args.batch, 40, 384, 30522, ragged=True)
    image, ids, atts = b["image"].to(dev), b["text_ids"].to(dev), b["text_atts"].to(dev)
    idx = (torch.arange(args.batch, device=dev) // 2).long()
    params = list(model.parameters())

    def step():
        for p in params:
            p.grad = None
        loss_itc, loss_itm = model(image, ids, atts, idx=idx)
        (loss_itc + loss_itm).backward()
        return loss_itc.detach(), loss_itm.detach()

    med, lo, hi = timed(torch, step, args.steps, args.warmup)
    out.update(eager_ms_per_step=round(med, 2), eager_ms_min_max=[round(lo, 2), round(hi, 2)])
    gstep = graph.GraphedStep(step)
    out["graph_mode"] = gstep.mode
    med, lo, hi = timed(torch, gstep, args.steps, args.warmup)
    out.update(graphed_ms_per_step=round(med, 2), graphed_ms_min_max=[round(lo, 2), round(hi, 2)], pairs_per_s=round(args.batch * 1000.0 / med, 1))
    loss_itc, loss_itm = gstep()
    print(json.dumps(dict({"probe": "retrieval train step (fwd+bwd)", "geometry": "BEiT2-large 384px + BERT-large 12+6 layers, batch %d (ids b // 2), "
                           "40 tokens, train mode" % args.batch, "steps": args.steps, "warmup": args.warmup,
                           "loss_itc": round(float(loss_itc), 5), "loss_itm": round(float(loss_itm), 5),
                           "no_negative_rows": int(model.last_no_negative.sum())}, **out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--itc-steps", type=int, default=200)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--captions", type=int, default=25010)
    ap.add_argument("--recall-repeats", type=int, default=5)
    ap.add_argument("--skip-step", action="store_true")
    bench(ap.parse_args())


if __name__ == "__main__":
    main()
