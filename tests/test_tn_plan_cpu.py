"""x2_tn_plan, the host planner of a weight-gradient queue (csrc/gemm.hip), through ctypes without a GPU: every tile of every problem is
covered exactly once by windows that stay inside their problem, at most 32 windows per launch, whole rounds of the compute units unsplit,
only the tiles left over split - by slices of at least 16 contraction steps and within the workspace offered."""
import importlib

import pytest

VIS = [(12608, 768, 3072), (12608, 3072, 768), (12608, 768, 768), (12608, 2304, 768)]                 # a BEiT-2 base block: 108 tiles
FUS = [(12608, 1536, 768), (7680, 768, 3072), (7680, 3072, 768), (7680, 768, 768), (7680, 768, 768), (7680, 768, 768),
       (7680, 2304, 768)]                                                                             # a fusion layer: 144 tiles
LARGE = [(18464, 1024, 4096), (18464, 4096, 1024), (18464, 1024, 1024), (18464, 3072, 1024)]          # an X2VLM-large block: 192 tiles
QUEUES = {
    "base_vision_pair": VIS * 2,
    "six_fusion_layers": FUS * 6,
    "large_pair": LARGE * 2,
    "nine_tiles": [(12544, 768, 768)],
    "more_than_a_round": [(1920, 30528, 768)],                                                        # 360 tiles
    "ragged_and_many": [(1154, 264, 520)] * 40 + [(200, 256, 256)] * 37,                              # more than 32 problems in a round
}
WS = {"room": 4 * 255 * 65536, "tight": 100 * 65536, "none": 0}


def tiles_of(shape):
    return ((shape[1] + 255) // 256) * ((shape[2] + 255) // 256)


@pytest.mark.parametrize("cus", [256, 240, 8, 1])
@pytest.mark.parametrize("ws", sorted(WS))
@pytest.mark.parametrize("queue", sorted(QUEUES))
def test_plan_covers_every_tile_once_in_whole_rounds(queue, ws, cus):
    K = importlib.import_module("x2-vlm_amd.kernels")
    shapes, ws_floats = QUEUES[queue], WS[ws]
    windows, launches = K.tn_plan(shapes, cus=cus, ws_floats=ws_floats)
    total = sum(tiles_of(s) for s in shapes)
    # windows stay inside their problem, walk the problems and each problem's tiles in order, and cover every tile exactly once
    seen = [0] * len(shapes)
    order = []
    for launch, prob, first, n in windows:
        assert 0 <= prob < len(shapes) and n >= 1 and 0 <= launch < len(launches)
        assert first == seen[prob], "problem %d: window starts at tile %d, %d tiles handed out so far" % (prob, first, seen[prob])
        seen[prob] += n
        assert seen[prob] <= tiles_of(shapes[prob])
        order.append((launch, prob))
    assert seen == [tiles_of(s) for s in shapes]
    assert order == sorted(order)
    per_launch = [[w for w in windows if w[0] == l] for l in range(len(launches))]
    assert all(1 <= len(w) <= 32 for w in per_launch)
    # whole rounds unsplit, the rest in remainder launches that come last
    main = sum(n for l, _, _, n in windows if not launches[l][1])
    rest = sum(n for l, _, _, n in windows if launches[l][1])
    assert main == total // cus * cus and rest == total % cus and main % cus == 0
    flags = [r for _, r in launches]
    assert flags == sorted(flags)
    for (split, rem), wins in zip(launches, per_launch):
        t = sum(w[3] for w in wins)
        if not rem:
            assert split == 1
            continue
        assert 1 <= split <= 4
        if split > 1:
            assert split * t * 65536 <= ws_floats
            for _, prob, _, _ in wins:
                steps = (shapes[prob][0] + 63) // 64
                assert steps // split >= 16, "a slice of %d steps cut in %d" % (steps, split)
    # one remainder launch unless its windows exceed 32
    assert sum(flags) <= 1 or queue == "ragged_and_many"


def test_plan_of_the_step_queues():
    """The numbers the callers rely on, at 256 compute units: six fusion layers = 3 unsplit rounds + 96 tiles in 2 slices; a queue that fits one
    round is one launch under the rule of x2_gemm_tn_grouped (a fusion layer alone: 3 slices, a vision pair: none)."""
    K = importlib.import_module("x2-vlm_amd.kernels")
    room = WS["room"]
    windows, launches = K.tn_plan(FUS * 6, cus=256, ws_floats=room)
    assert launches[-1] == (2, 1) and all(l == (1, 0) for l in launches[:-1])
    assert sum(n for l, _, _, n in windows if launches[l][1]) == 96
    # 37 windows of unsplit tiles need two launches: the first ends at a whole round (512), not where its 32 entries run out (675)
    assert [sum(n for l, _, _, n in windows if l == i) for i in range(len(launches))] == [512, 256, 96]
    assert K.tn_plan(FUS, cus=256, ws_floats=room)[1] == [(3, 1)]
    assert K.tn_plan(VIS * 2, cus=256, ws_floats=room)[1] == [(1, 1)]
    assert K.tn_plan(FUS, cus=256, ws_floats=0)[1] == [(1, 1)]
    # a window that begins in the middle of a problem: problem 8 of the queue is cut at the end of the first round
    cut = [w for w in windows if w[2] > 0]
    assert cut and all(w[0] > 0 for w in cut)


def test_plan_refuses_bad_arguments():
    K = importlib.import_module("x2-vlm_amd.kernels")
    with pytest.raises(RuntimeError, match="x2_tn_plan"):
        K.tn_plan([(0, 256, 256)], cus=256)
    with pytest.raises(RuntimeError, match="x2_tn_plan"):
        K.tn_plan([(64, 256, -4)], cus=256)
