"""Data parallelism of the real step, observed on the 1-GPU box.

(a) Two ranks sharing GPU 0 (gloo rendezvous: RCCL refuses two ranks on one device) run the real
    x2-vlm_amd XVLM step through RocmDDPAccelerator on two different half-batches.  The averaged gradients must equal
    what the CPU oracle gives for the same two half-batches under the reference's semantics (SURVEY.md 8e,
    xvlm.py:140-160, 805-826, apex DDP averaging): every rank evaluates the ITC loss over the all-gathered
    features but back-propagates only through its own rows; ITM / MLM are per-rank means; gradients are averaged.
    Includes the reference's two-backward_step-per-iteration pattern (Pretrain.py:197, 247).
(b) A single-rank RCCL process group (backend "nccl") goes through set_up / broadcast / backward_step /
    optimizer_step and the ITC all-gather, so the RCCL code path has executed on hardware.

Tolerances as tests/test_model_gpu.py (bf16 operands vs the fp32 oracle)."""
import importlib
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from cases import CASES, model_config
from ddp_helpers import _compare

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_batch(synthetic, c, rank, shift=0):
    seed = c["bseed"] + 100 * rank + shift
    b = synthetic.synth_batch(seed, c["batch"], c["seq_len"], c["image_res"], c["vocab"], c["max_masks"], ragged=c["ragged"],
                              frames=c["frames"])
    return b, synthetic.synth_negatives(seed, c["batch"])


def _step(model, batch, neg):
    model.injected_negatives = neg
    loss = model(batch["image"], batch["text_ids"], batch["text_atts"], text_ids_masked=batch["text_ids_masked"],
                 masked_pos=batch["masked_pos"], masked_ids=batch["masked_ids"])
    return loss, sum(loss.values())


def _two_rank_worker(rank, world, port, case, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), X2_DIST_BACKEND="gloo")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    mp_ = importlib.import_module("x2-vlm_amd.model_pretrain")
    acc = importlib.import_module("x2-vlm_amd.accelerator")
    c = CASES[case]
    model = mp_.XVLM(config=model_config(case, tempfile.mkdtemp()), load_vision_params=False, load_text_params=False, pretraining=True)
    synthetic.synth_state_dict(model, c["wseed"])
    model.eval()
    a = acc.RocmDDPAccelerator(dict(RNG_SEED=7), None)
    ddp, _, _ = a.set_up(model, None, None, local_rank=0, world_size=world, rank=rank)
    try:
        out = {}
        b1, n1 = _rank_batch(synthetic, c, rank)
        b2, n2 = _rank_batch(synthetic, c, rank, shift=1000)
        b1 = {k: v.cuda() for k, v in b1.items()}
        b2 = {k: v.cuda() for k, v in b2.items()}
        loss, total = _step(ddp.module, b1, n1)
        a.backward_step(total, None)
        torch.cuda.synchronize()
        out["loss1"] = {k: float(v) for k, v in loss.items()}
        out["g1"] = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
        out["early"] = a.buckets.messages
        _, total = _step(ddp.module, b2, n2)               # second backward_step, gradients accumulate
        a.backward_step(total, None)
        torch.cuda.synchronize()
        out["g2"] = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
        ret[rank] = out
    finally:
        a.buckets.close()
        dist.destroy_process_group()


def _oracle_ddp(synthetic, c, world, shift):
    """Averaged gradients + per-rank losses of `world` ranks under the reference's DDP semantics, on the CPU oracle."""
    from oracle import x2vlm_oracle as O
    cfg = O.config_from_case(c)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    sd = O.make_params(cfg, c["wseed"], synthetic.synth_tensor)
    data = [_rank_batch(synthetic, c, r, shift) for r in range(world)]
    feats = []
    with torch.no_grad():
        for b, n in data:
            _, ex = O.xvlm_forward(sd, cfg, b, n)
            feats.append((ex["image_feat"].detach(), ex["text_feat"].detach()))
    avg, losses = {}, []
    for r, (b, n) in enumerate(data):
        for t in sd.values():
            t.grad = None
        calls = []

        def gather(t, r=r, calls=calls):
            which = len(calls)                              # first call: image features, second: text features
            calls.append(1)
            return torch.cat([t if q == r else feats[q][which] for q in range(world)])
        loss, _ = O.xvlm_forward(sd, cfg, b, n, gather=gather)
        sum(loss.values()).backward()
        losses.append({k: float(v) for k, v in loss.items()})
        for k, t in sd.items():
            if t.grad is not None:
                avg[k] = avg.get(k, 0) + t.grad.detach().clone() / world
    return avg, losses


@pytest.mark.parametrize("case", ["tiny", "base_shallow"])
def test_two_ranks_match_oracle_ddp_semantics(case, synthetic):
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_two_rank_worker, args=(world, _free_port(), case, ret), nprocs=world, join=True)
    out = [ret[r] for r in range(world)]
    c = CASES[case]
    g_a, loss_a = _oracle_ddp(synthetic, c, world, 0)
    g_b, _ = _oracle_ddp(synthetic, c, world, 1000)
    for r in range(world):
        for k, v in loss_a[r].items():                      # ITC is the GLOBAL loss: identical on both ranks
            assert abs(out[r]["loss1"][k] - v) <= 5e-3 * max(abs(v), 1e-6), (r, k, out[r]["loss1"][k], v)
        assert out[r]["early"] >= 3                         # per-layer arenas went out early, plus the leftover bucket
        _compare(out[r]["g1"], g_a, "rank %d, one backward_step" % r)
        _compare(out[r]["g2"], {k: g_a[k] + g_b[k] for k in g_a}, "rank %d, two backward_steps" % r)
    assert abs(loss_a[0]["loss_itc"] - loss_a[1]["loss_itc"]) < 1e-6
    for n in out[0]["g2"]:                                  # replicas end up with the same gradients
        assert torch.allclose(out[0]["g2"][n], out[1]["g2"][n], rtol=1e-5, atol=1e-7), n


def _two_rank_segmented_worker(rank, world, port, case, ret, env=None):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), X2_DIST_BACKEND="gloo")
    os.environ.update(env or {})
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    mp_ = importlib.import_module("x2-vlm_amd.model_pretrain")
    acc = importlib.import_module("x2-vlm_amd.accelerator")
    c = CASES[case]
    model = mp_.XVLM(config=model_config(case, tempfile.mkdtemp()), load_vision_params=False, load_text_params=False, pretraining=True)
    synthetic.synth_state_dict(model, c["wseed"])
    model.eval()
    a = acc.RocmDDPAccelerator(dict(RNG_SEED=7), None)
    ddp, _, _ = a.set_up(model, None, None, local_rank=0, world_size=world, rank=rank)
    try:
        out = {}
        b1, n1 = _rank_batch(synthetic, c, rank)
        b2, n2 = _rank_batch(synthetic, c, rank, shift=1000)
        static = {k: v.cuda() for k, v in b1.items()}
        neg = [torch.tensor(n, dtype=torch.int32, device="cuda") for n in n1]
        model.injected_negatives = tuple(neg)
        step = a.segmented_step(ddp, static, clamp_temp=False)
        out["mode"], out["error"] = step.mode, step.error
        out["aux"], out["bf16"], out["reserved"] = step.aux_overlap, step.grad_bf16, step.reserved_cus
        loss = step()
        torch.cuda.synchronize()
        out["loss1"] = {k: float(v) for k, v in loss.items()}
        out["g1"] = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
        out["messages"] = step.messages
        # a second iteration on new data through the SAME graphs: static inputs are overwritten, gradients are rewritten
        step.copy_inputs(static, {k: v.cuda() for k, v in b2.items()})
        for t, n in zip(neg, n2):
            t.copy_(torch.tensor(n, dtype=torch.int32))
        for p in model.parameters():
            p.grad = None                                    # what optimizer.zero_grad(set_to_none=True) does between iterations
        step()
        torch.cuda.synchronize()
        out["g2"] = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
        ret[rank] = out
    finally:
        a.buckets.close()
        dist.destroy_process_group()


@pytest.mark.parametrize("case", ["tiny", "base_shallow"])
def test_two_ranks_replayed_segments_match_oracle_ddp_semantics(case, synthetic):
    """The N > 1 step as REPLAYED hipGraph segments (graph.SegmentedStep through RocmDDPAccelerator.segmented_step): ITC
    all-gather between two segments, per-segment gradient all-reduces behind them.  Same oracle, same tolerances as the
    eager two-rank test above; two successive iterations through the same graphs."""
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_two_rank_segmented_worker, args=(world, _free_port(), case, ret), nprocs=world, join=True)
    out = [ret[r] for r in range(world)]
    c = CASES[case]
    g_a, loss_a = _oracle_ddp(synthetic, c, world, 0)
    g_b, _ = _oracle_ddp(synthetic, c, world, 1000)
    for r in range(world):
        assert out[r]["mode"] == "hipgraph-segments", out[r]["error"]
        for k, v in loss_a[r].items():
            assert abs(out[r]["loss1"][k] - v) <= 5e-3 * max(abs(v), 1e-6), (r, k, out[r]["loss1"][k], v)
        assert out[r]["messages"] >= 2 + 3                  # two feature gathers + at least one message per gradient segment
        _compare(out[r]["g1"], g_a, "rank %d, first replay" % r)
        _compare(out[r]["g2"], g_b, "rank %d, second replay (new data)" % r)
    for n in out[0]["g2"]:                                  # replicas end up with the same gradients
        assert torch.allclose(out[0]["g2"][n], out[1]["g2"][n], rtol=1e-5, atol=1e-7), n


@pytest.mark.parametrize("world,case,bf16", [(4, "tiny", False), (8, "base_shallow", False), (2, "tiny", True), (8, "tiny", True)])
def test_many_ranks_replayed_segments_match_oracle_ddp_semantics(world, case, bf16, synthetic):
    """BASELINE.json configs[2] is 8 ranks: the replayed step at 4 and 8 ranks sharing this GPU over gloo (RCCL refuses two ranks
    on one device) - on the toy model and, at 8 ranks, at the real token geometry (base_shallow: N = 197, V = 30522).  Every rank
    derives its reduction plan from its own capture - SegmentedStep compares the plans' digests at set-up and raises on a
    mismatch instead of hanging; here: mode, message count equal on all ranks, losses and averaged gradients equal to the
    oracle's W-rank semantics (global ITC loss over W * B gathered pairs, local rows attached).
    bf16: X2_GRAD_BF16=1, the gradient arenas travel as bf16 (0.51 GB per step) and are averaged in bf16, fp32 at both
    ends - same bounds (one more bf16 rounding per hop on top of the bf16 operands' noise), replicas still bit-identical.
    With collectives in the step the tail segment's forked stream is off by default (host thread free for the collectives)."""
    mgr = mp.Manager()
    ret = mgr.dict()
    env = dict(X2_GRAD_BF16="1" if bf16 else "0")
    mp.spawn(_two_rank_segmented_worker, args=(world, _free_port(), case, ret, env), nprocs=world, join=True)
    out = [ret[r] for r in range(world)]
    c = CASES[case]
    g_a, loss_a = _oracle_ddp(synthetic, c, world, 0)
    big = case != "tiny"
    g_b = None if big else _oracle_ddp(synthetic, c, world, 1000)[0]       # real geometry: the oracle's 8 ranks once (CPU time)
    assert len(set(o["messages"] for o in out)) == 1
    for r in range(world):
        assert out[r]["mode"] == "hipgraph-segments", out[r]["error"]
        assert out[r]["aux"] is False and out[r]["bf16"] is bf16
        for k, v in loss_a[r].items():
            assert abs(out[r]["loss1"][k] - v) <= 5e-3 * max(abs(v), 1e-6), (r, k, out[r]["loss1"][k], v)
        _compare(out[r]["g1"], g_a, "rank %d of %d, first replay" % (r, world))
        if g_b is not None:
            _compare(out[r]["g2"], g_b, "rank %d of %d, second replay (new data)" % (r, world))
    for r in range(1, world):
        for n in out[0]["g2"]:
            assert torch.allclose(out[0]["g2"][n], out[r]["g2"][n], rtol=1e-5, atol=1e-7), (r, n)


def _plan_mismatch_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), X2_DIST_BACKEND="gloo")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    mp_ = importlib.import_module("x2-vlm_amd.model_pretrain")
    acc = importlib.import_module("x2-vlm_amd.accelerator")
    graph = importlib.import_module("x2-vlm_amd.graph")
    c = CASES["tiny"]
    model = mp_.XVLM(config=model_config("tiny", tempfile.mkdtemp()), load_vision_params=False, load_text_params=False, pretraining=True)
    synthetic.synth_state_dict(model, c["wseed"])
    model.eval()
    a = acc.RocmDDPAccelerator(dict(RNG_SEED=7), None)
    ddp, _, _ = a.set_up(model, None, None, local_rank=0, world_size=world, rank=rank)
    try:
        b1, n1 = _rank_batch(synthetic, c, rank)
        static = {k: v.cuda() for k, v in b1.items()}
        model.injected_negatives = tuple(torch.tensor(n, dtype=torch.int32, device="cuda") for n in n1)
        if rank == 1:       # this rank's plan gets one more message than the others'
            orig = graph.SegmentedStep._plan_digest
            graph.SegmentedStep._plan_digest = lambda self: (orig(self)[0] ^ 1, orig(self)[1] + 1)
        try:
            a.segmented_step(ddp, static, clamp_temp=False)
            ret[rank] = "no error"
        except RuntimeError as e:
            ret[rank] = str(e)
    finally:
        a.buckets.close()
        dist.destroy_process_group()


def test_ranks_with_different_reduction_plans_raise_instead_of_hanging():
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_plan_mismatch_worker, args=(2, _free_port(), ret), nprocs=2, join=True)
    for r in range(2):
        assert "different gradient-reduction plans" in ret[r], ret[r]


def _rccl_segmented_worker(rank, world, port, ret, comm_mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), X2_DDP_SINGLE_RANK_COLLECTIVES="1", X2_COMM=comm_mode)
    os.environ.pop("X2_DIST_BACKEND", None)
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    mp_ = importlib.import_module("x2-vlm_amd.model_pretrain")
    acc = importlib.import_module("x2-vlm_amd.accelerator")
    c = CASES["tiny"]
    model = mp_.XVLM(config=model_config("tiny", tempfile.mkdtemp()), load_vision_params=False, load_text_params=False, pretraining=True)
    synthetic.synth_state_dict(model, c["wseed"])
    model.eval()
    a = acc.RocmDDPAccelerator(dict(RNG_SEED=7), None)
    ddp, _, _ = a.set_up(model, None, None, local_rank=0, world_size=1, rank=0)
    try:
        assert dist.get_backend() == "nccl" and (a.buckets.comm is not None) == (comm_mode == "rccl")
        b, n = _rank_batch(synthetic, c, 0)
        static = {k: v.cuda() for k, v in b.items()}
        model.injected_negatives = tuple(torch.tensor(x, dtype=torch.int32, device="cuda") for x in n)
        step = a.segmented_step(ddp, static, clamp_temp=False)
        loss = step()
        torch.cuda.synchronize()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        msgs = step.messages
        # the same step with no collective anywhere
        a.buckets.close()
        os.environ["X2_DDP_SINGLE_RANK_COLLECTIVES"] = "0"
        for p in model.parameters():
            p.grad = None
        model.injected_negatives = n
        _, total = _step(model, static, n)
        total.backward()
        torch.cuda.synchronize()
        worst = max(float((grads[k] - p.grad).abs().max()) / (float(p.grad.abs().max()) + 1e-12)
                    for k, p in model.named_parameters() if p.grad is not None)
        ret[0] = dict(mode=step.mode, error=step.error, msgs=msgs, worst=worst, losses={k: float(v) for k, v in loss.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("comm_mode", ["torch", "rccl"])
def test_single_rank_rccl_through_replayed_segments(comm_mode):
    """Both collective back-ends (torch.distributed "nccl" = RCCL, and the C-ABI communicator x2_comm_*) driven by the REPLAYED
    step: ITC all-gathers between segments, per-segment AVG all-reduces on the collective stream, the plan-digest exchange at
    set-up.  One rank (the box has one GPU): averaging is the identity, so the gradients must equal the plain eager step's up
    to the run-to-run noise of the atomics."""
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rccl_segmented_worker, args=(1, _free_port(), ret, comm_mode), nprocs=1, join=True)
    r = ret[0]
    assert r["mode"] == "hipgraph-segments", r["error"]
    assert r["msgs"] >= 2 + 3
    assert all(np.isfinite(v) for v in r["losses"].values())
    assert r["worst"] <= 2e-2, r["worst"]


def _mixed_rank_data(synthetic, c, rank, shift=0):
    si = c["bseed"] + 100 * rank + shift
    sr = si + 7
    bi = synthetic.synth_batch(si, 4, c["seq_len"], c["image_res"], c["vocab"], c["max_masks"], ragged=True)
    br = synthetic.synth_region_batch(sr, c["n_images"], c["batch"], c["seq_len"], c["image_res"], 16, c["vocab"], c["max_masks"])
    return (bi, synthetic.synth_negatives(si, 4)), (br, synthetic.synth_negatives(sr, c["batch"]))


def _two_rank_mixed_worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), X2_DIST_BACKEND="gloo")
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    mp_ = importlib.import_module("x2-vlm_amd.model_pretrain")
    acc = importlib.import_module("x2-vlm_amd.accelerator")
    c = CASES["tiny_region"]
    model = mp_.XVLM(config=model_config("tiny_region", tempfile.mkdtemp()), load_vision_params=False, load_text_params=False, pretraining=True)
    synthetic.synth_state_dict(model, c["wseed"])
    model.eval()
    a = acc.RocmDDPAccelerator(dict(RNG_SEED=7), None)
    ddp, _, _ = a.set_up(model, None, None, local_rank=0, world_size=world, rank=rank)
    try:
        out = {}
        (bi, ni), (br, nr) = _mixed_rank_data(synthetic, c, rank)
        si, sr = {k: v.cuda() for k, v in bi.items()}, {k: v.cuda() for k, v in br.items()}
        negi = tuple(torch.tensor(n, dtype=torch.int32, device="cuda") for n in ni)
        negr = tuple(torch.tensor(n, dtype=torch.int32, device="cuda") for n in nr)
        step = a.mixed_step(ddp, [dict(batch=si, negatives=negi), dict(batch=sr, negatives=negr, weight=0.5, ret_bbox_loss=True)],
                            clamp_temp=False)
        out["mode"], out["error"] = step.mode, step.error
        for it in range(2):
            if it:
                (bi, ni), (br, nr) = _mixed_rank_data(synthetic, c, rank, shift=1000)
                step.copy_inputs(0, {k: v.cuda() for k, v in bi.items()})
                step.copy_inputs(1, {k: v.cuda() for k, v in br.items()})
                for t, n in zip(negi + negr, list(ni) + list(nr)):
                    t.copy_(torch.tensor(n, dtype=torch.int32))
                for p in model.parameters():
                    p.grad = None
            li, lr = step()
            torch.cuda.synchronize()
            out["loss%d" % it] = ({k: float(v) for k, v in li.items()}, {k: float(v) for k, v in lr.items()})
            out["g%d" % it] = {n: p.grad.detach().cpu() for n, p in model.named_parameters() if p.grad is not None}
            out["messages%d" % it] = step.messages
        ret[rank] = out
    finally:
        a.buckets.close()
        dist.destroy_process_group()


def _oracle_ddp_mixed(synthetic, c, world, shift):
    """Averaged accumulated gradients of `world` ranks: image part + 0.5 x region part, each under the reference's DDP semantics
    (global ITC loss over the gathered features, local rows attached)."""
    from oracle import x2vlm_oracle as O
    cfg = O.config_from_case(c)
    torch.set_num_threads(min(os.cpu_count() or 1, 32))
    sd = O.make_params(cfg, c["wseed"], synthetic.synth_tensor)
    data = [_mixed_rank_data(synthetic, c, r, shift) for r in range(world)]
    avg, losses = {}, []
    for part, (w, kw) in enumerate(((1.0, {}), (0.5, dict(ret_bbox_loss=True)))):
        feats = []
        with torch.no_grad():
            for d in data:
                _, ex = O.xvlm_forward(sd, cfg, d[part][0], d[part][1], **kw)
                feats.append((ex["image_feat"].detach(), ex["text_feat"].detach()))
        for r, d in enumerate(data):
            for t in sd.values():
                t.grad = None
            calls = []

            def gather(t, r=r, calls=calls, feats=feats):
                which = len(calls)
                calls.append(1)
                return torch.cat([t if q == r else feats[q][which] for q in range(world)])
            loss, _ = O.xvlm_forward(sd, cfg, d[part][0], d[part][1], gather=gather, **kw)
            (w * sum(loss.values())).backward()
            losses.append((part, r, {k: float(v) for k, v in loss.items()}))
            for k, t in sd.items():
                if t.grad is not None:
                    avg[k] = avg.get(k, 0) + t.grad.detach().clone() / world
    return avg, losses


def test_two_ranks_replayed_mixed_iteration_matches_oracle(synthetic):
    """Pretrain.run_mixed_iter at two ranks as replayed segments (RocmDDPAccelerator.mixed_step -> graph.MixedStep): image part +
    region part (iter_perc 0.5), gradients accumulated in static buffers, ONE averaging per arena after the second part; two
    successive iterations through the same graphs against the oracle's accumulated two-rank gradients."""
    world = 2
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_two_rank_mixed_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    out = [ret[r] for r in range(world)]
    c = CASES["tiny_region"]
    for it, shift in enumerate((0, 1000)):
        want, losses = _oracle_ddp_mixed(synthetic, c, world, shift)
        for part, r, ref in losses:
            for k, v in ref.items():
                got = out[r]["loss%d" % it][part][k]
                assert abs(got - v) <= 5e-3 * max(abs(v), 1.0), (it, part, r, k, got, v)
        for r in range(world):
            assert out[r]["mode"] == "hipgraph-segments", out[r]["error"]
            # pointwise bound 1.2e-1 (8e-2 for a single iteration; measured 8.3e-2 on one cancellation-dominated key weight):
            # the sum of two sub-iterations' bf16 noise
            _compare(out[r]["g%d" % it], want, "rank %d, mixed iteration %d" % (r, it), etol=1.2e-1)
            assert "bbox_head.0.weight" in out[r]["g%d" % it]
        assert out[0]["messages%d" % it] == out[1]["messages%d" % it]
        # 2 + 2 feature gathers; the gradient messages of ONE reduction plan (not one per part)
        assert 4 + 3 <= out[0]["messages%d" % it] <= 4 + 30, out[0]["messages%d" % it]
        for n in out[0]["g%d" % it]:
            assert torch.allclose(out[0]["g%d" % it][n], out[1]["g%d" % it][n], rtol=1e-5, atol=1e-7), n


def _rccl_worker(rank, world, port, ret, comm_mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), X2_DDP_SINGLE_RANK_COLLECTIVES="1", X2_COMM=comm_mode)
    os.environ.pop("X2_DIST_BACKEND", None)
    synthetic = importlib.import_module("x2-vlm_amd.synthetic")
    mp_ = importlib.import_module("x2-vlm_amd.model_pretrain")
    acc = importlib.import_module("x2-vlm_amd.accelerator")
    optim = importlib.import_module("x2-vlm_amd.optim")
    xvlm = importlib.import_module("x2-vlm_amd.xvlm")
    c = CASES["tiny"]
    model = mp_.XVLM(config=model_config("tiny", tempfile.mkdtemp()), load_vision_params=False, load_text_params=False, pretraining=True)
    synthetic.synth_state_dict(model, c["wseed"])
    model.eval()
    opt = optim.create_optimizer(dict(lr=1e-4, weight_decay=0.01, lr_mult=2), model)
    a = acc.RocmDDPAccelerator(dict(RNG_SEED=7), None)
    ddp, opt, _ = a.set_up(model, opt, None, local_rank=0, world_size=1, rank=0)
    try:
        assert dist.get_backend() == "nccl" and (a.buckets.comm is not None) == (comm_mode == "rccl")
        b, n = _rank_batch(synthetic, c, 0)
        b = {k: v.cuda() for k, v in b.items()}
        loss, total = _step(ddp.module, b, n)
        a.backward_step(total, opt)
        msgs = a.buckets.messages
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        # the ITC all-gather on RCCL (allgather() short-cuts a single rank, so call the Function directly)
        t = torch.randn(4, 8, device="cuda", requires_grad=True)
        y = xvlm.AllGather.apply(t, 0, 1)
        y.sum().backward()
        before = model.vision_proj.weight.detach().clone()
        norm = a.optimizer_step(opt, ddp, 1.0)
        opt.step()
        torch.cuda.synchronize()
        moved = float((model.vision_proj.weight.detach() - before).abs().max()) > 0.0
        # the same step without any process group in the way
        for p in model.parameters():
            p.grad = None
        synthetic.synth_state_dict(model, c["wseed"])
        a.buckets.close()
        _, total = _step(model, b, n)
        total.backward()
        torch.cuda.synchronize()
        worst = max(float((grads[k] - p.grad).abs().max()) / (float(p.grad.abs().max()) + 1e-12)
                    for k, p in model.named_parameters() if p.grad is not None)
        ret[0] = dict(msgs=msgs, norm=norm, gather_ok=bool(torch.equal(y.detach(), t.detach()) and torch.equal(t.grad, torch.ones_like(t))),
                      moved=moved, worst=worst,
                      losses={k: float(v) for k, v in loss.items()})
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("comm_mode", ["torch", "rccl"])
def test_single_rank_rccl_through_the_accelerator(comm_mode):
    """comm_mode torch: torch.distributed backend "nccl" (= RCCL); rccl: the C-ABI communicator x2_comm_* for the buckets."""
    mgr = mp.Manager()
    ret = mgr.dict()
    mp.spawn(_rccl_worker, args=(1, _free_port(), ret, comm_mode), nprocs=1, join=True)
    r = ret[0]
    assert r["msgs"] >= 3 and r["gather_ok"] and r["moved"]      # the optimizer step changed the weights
    assert np.isfinite(r["norm"]) and r["norm"] > 0
    assert all(np.isfinite(v) for v in r["losses"].values())
    assert r["worst"] <= 1e-6, r["worst"]                   # AVG over one rank is the identity


def test_c_abi_communicator_single_rank():
    """x2_comm_* (include/x2vlm_hip.h) on a one-rank RCCL communicator: every entry point runs on the device."""
    comm = importlib.import_module("x2-vlm_amd.comm")
    c = comm.X2Comm(comm.X2Comm.unique_id(), 0, 1)
    assert c.info() == (0, 1)
    side = torch.cuda.Stream()
    x = torch.randn(1 << 20, device="cuda")
    want = x.clone()
    side.wait_stream(torch.cuda.current_stream())
    ev = c.allreduce_bucket(x, average=True, stream=side, want_event=True)
    ev.synchronize()
    assert torch.equal(x, want)
    xb = torch.randn(4096, device="cuda").bfloat16()
    wb = xb.clone()
    c.allreduce_bucket(xb, average=False)
    out = torch.empty(64 * 256, device="cuda")
    feat = torch.randn(64, 256, device="cuda")
    c.allgather(feat, out)
    c.broadcast(x, root=0)
    torch.cuda.synchronize()
    assert torch.equal(xb, wb) and torch.equal(out.view(64, 256), feat) and torch.equal(x, want)
    c.destroy()
