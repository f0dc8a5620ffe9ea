"""engine.run_wgrad_queue on the host: the launches kernels.gemm_tn_queue makes are recorded instead of run (no GPU), with the real planner.
Every layer's pre-work comes before the first launch, a layer's post-work (layerscale_finish, GRAD_READY_HOOK) comes right behind the launch
that holds the last tile of its last problem - never before it - and every layer's post-work runs exactly once."""
import importlib

import pytest
import torch

CUS = 16
# (Mc, N, K) per problem, one list per layer: 9 + 8 + 6 + 11 = 34 tiles on 16 compute units = a launch of 32 unsplit tiles + 2 left over
LAYERS = [[(64, 512, 512), (192, 264, 264), (200, 256, 256)], [(64, 512, 264), (192, 512, 512)], [(64, 256, 512), (64, 512, 264)],
          [(200, 512, 512), (64, 264, 512), (192, 256, 264), (64, 256, 256)]]


def closure(events, i, shapes):
    def later():
        events.append(("alone", i))
    later.pre = lambda: events.append(("pre", i))
    later.post = lambda: events.append(("post", i))
    later.tn = [(torch.empty(mc, n, dtype=torch.bfloat16), torch.empty(mc, k, dtype=torch.bfloat16), torch.empty(n, k)) for mc, n, k in shapes]
    return later


@pytest.fixture
def recorded(monkeypatch):
    K = importlib.import_module("x2-vlm_amd.kernels")
    lib = importlib.import_module("x2-vlm_amd._lib")
    events = []

    def call(name, *args):
        assert name == "x2_gemm_tn_queue"
        events.append(("launch", args[5], args[6]))            # first_launch, n_launches
    monkeypatch.setattr(K, "call", call)
    monkeypatch.setattr(K, "workspace", lambda dev, n: torch.empty(1))      # never read: nothing is launched
    with lib.tuned({5: 2, 12: 256 - CUS}):                      # no device: the library plans with 256 compute units less the reservation
        yield K, events


def test_post_work_follows_the_launch_that_completes_the_layer(recorded):
    K, events = recorded
    eng = importlib.import_module("x2-vlm_amd.engine")
    shapes = [s for layer in LAYERS for s in layer]
    windows, launches = K.tn_plan(shapes, 0, 4 * 255 * 65536)
    assert len(launches) >= 2 and [r for _, r in launches][-1] == 1
    eng.run_wgrad_queue([closure(events, i, layer) for i, layer in enumerate(LAYERS)])
    n = len(LAYERS)
    assert events[:n] == [("pre", i) for i in range(n)]
    assert [e for e in events if e[0] == "launch"] == [("launch", l, 1) for l in range(len(launches))]
    assert sorted(e for e in events if e[0] == "post") == [("post", i) for i in range(n)] and not [e for e in events if e[0] == "alone"]
    last_problem, k = [], 0
    for layer in LAYERS:
        k += len(layer)
        last_problem.append(k - 1)
    for i in range(n):
        completing = max(l for l, p, _, _ in windows if p == last_problem[i])
        at = events.index(("post", i))
        before = [e[1] for e in events[:at] if e[0] == "launch"]
        assert before and before[-1] == completing, "layer %d: post-work behind launch %s, its last tile is in launch %d" % (i, before[-1:], completing)


def test_a_single_layer_and_an_empty_layer(recorded):
    K, events = recorded
    eng = importlib.import_module("x2-vlm_amd.engine")
    eng.run_wgrad_queue([closure(events, 0, LAYERS[0])])
    assert events == [("alone", 0)]
    eng.run_wgrad_queue(None)
    with pytest.raises(AssertionError, match="without weight-gradient problems"):
        eng.run_wgrad_queue([closure(events, 0, LAYERS[0]), closure(events, 1, [])])
