"""The two loops every fine-tune step test (test_nlvr_step_gpu.py, test_grounding_step_gpu.py, test_cls_wide_step_gpu.py) runs on a captured
graph.GraphedStep, with their bounds stated once.  tests/test_graph_gpu.py keeps its own copy of the first loop: the pretraining model has
parameters without a gradient, and carrying its None handling here would let a fine-tune step lose a gradient unnoticed."""
import importlib

import torch


def replays_match_eager(what, step, fwd_bwd, static, params, names, captured, data, before=None):
    """The captured step must BE the eager step: for every batch of `data` (copied into `static`) the eager launches of fwd_bwd and the replay of
    `step` run from the same state and agree to 1e-6 on every loss and to 5e-3 per gradient tensor, relative to max(its norm, 1e-2 * the norm of
    all gradients); every replayed gradient (`captured`: the arenas the graph writes) is finite.  Then the state moves by an SGD step.
    before(i, batch), if given, runs after the copy and before the eager launches; what it returns, if anything, is called with the replayed
    losses once the gradients have been compared.  Returns the replayed losses of every batch."""
    graph = importlib.import_module("x2-vlm_amd.graph")
    seen = []
    for i, b in enumerate(data):
        graph.GraphedStep.copy_inputs(static, b)
        after = before(i, b) if before is not None else None
        le = {k: float(v) for k, v in fwd_bwd().items()}     # eager launches (re-binds .grad to fresh tensors)
        torch.cuda.synchronize()
        eager = [p.grad.detach().clone() for p in params]
        lg = {k: float(v) for k, v in step().items()}        # the same state through the captured graph
        torch.cuda.synchronize()
        for k in le:
            assert abs(le[k] - lg[k]) <= 1e-6 * max(1.0, abs(le[k])), (i, k, le[k], lg[k])
        total = sum(float(g.double().pow(2).sum()) for g in eager) ** 0.5
        worst = 0.0
        for n, ge, gg in zip(names, eager, captured):
            assert bool(torch.isfinite(gg).all()), n
            if "key.bias" not in n:                          # key biases: analytically zero gradient, pure rounding noise
                err = float((ge.double() - gg.double()).norm()) / max(float(ge.double().norm()), 1e-2 * total)
                worst = max(worst, err)
                assert err <= 5e-3, (i, n, err)
        if after is not None:
            after(lg)
        print("%s, batch %d: eager %s, replay %s, worst gradient tensor difference %.2e" % (what, i, le, lg, worst))
        seen.append(lg)
        with torch.no_grad():                                # the next state, through p.data as transformers' AdamW moves it
            for p, g in zip(params, eager):
                p.data.add_(g, alpha=-0.02)
    return seen


def replays_draw_new_masks(step, params):
    """Four replays of a train-mode step on constant inputs: every gradient and loss stays finite (and below 1e4), and the four loss tuples
    differ, i.e. every replay drew its own dropout masks."""
    seen = []
    for _ in range(4):
        loss = step()
        seen.append(tuple(round(float(v), 6) for v in loss.values()))
        assert all(bool(torch.isfinite(p.grad).all()) for p in params)
    assert all(all(x == x and abs(x) < 1e4 for x in s) for s in seen)   # finite
    assert len(set(seen)) == 4, seen                                    # same inputs, four different masks
