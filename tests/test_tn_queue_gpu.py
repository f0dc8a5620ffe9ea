"""x2_gemm_tn_queue (csrc/gemm.hip): a queue of weight-gradient problems run as whole rounds of the compute units plus one split remainder.
The 256x256 kernel is forced (knob 5 = 2) and all but 16 compute units are reserved (knob 12), so that queues of a few small problems
already have launch windows that begin and end inside a problem, a problem finished by two launches, more than 8 problems in one call and
a split remainder.  Every result is held to a float64 matmul at the bound tests/test_kernels_gpu.py uses for gemm_tn_grouped (1e-5 of
max-abs), every tile of an unsplit launch is the same integers as gemm_tn_grouped(split=1) of its problem alone, two runs give the same
integers, and nothing outside dW[N][K] (rows 4 floats apart from the next) or the workspace offered is written.

Shapes: N, K in {256, 264, 512} (264: the ragged edge, 2 tiles of which one is 8 wide), Mc in {64, 192, 200} (200: the ragged-contraction
instantiation).  The split rule never cuts a contraction into slices of fewer than 16 steps of 64, so the two split-remainder queues use
Mc = 2048 (32 steps: 2 slices) and Mc = 3080 (49 steps, ragged: 3 slices) at the same N and K."""
import ctypes as C

import pytest
import torch

from kernel_helpers import _ALIVE, F32, I32, K, bf, filled, guarded, lib, relerr, rnd, tuned  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
CUS = 16
# (Mc, N, K) per problem; tiles per problem in the comment
QUEUES = {
    # 25 tiles, 9 problems: round of 16 ends after 3 of problem 4's 4 tiles; the other 9 tiles are an unsplit remainder (4 steps at most)
    "nine_problems": [(64, 512, 512), (192, 264, 264), (200, 512, 264), (200, 256, 256), (64, 264, 512), (192, 256, 512), (200, 264, 256),
                      (64, 256, 264), (192, 512, 256)],
    # 22 tiles: the round ends after 2 of problem 4's tiles, remainder 6 tiles x 2 slices (12 of 16 slots; 3 slices: 18 of 32)
    "split2": [(2048, 512, 512), (2048, 264, 264), (2048, 512, 264), (2048, 256, 512), (2048, 264, 512), (2048, 512, 512)],
    # 21 tiles: remainder 5 tiles x 3 slices (15 of 16 slots)
    "split3": [(3080, 512, 512), (3080, 264, 264), (3080, 512, 264), (3080, 256, 512), (3080, 264, 512), (3080, 512, 256), (3080, 256, 256)],
    # 34 tiles: two whole rounds in one unsplit launch, the last problem begins in it and ends in the remainder of 2
    "two_rounds": [(200, 256, 512)] + [(200, 512, 512)] * 2 + [(64, 512, 512), (192, 512, 264)] * 3,
}
WANT_SPLIT = {"nine_problems": 1, "split2": 2, "split3": 3, "two_rounds": 1}
CUT = {"nine_problems": 4, "split2": 4, "split3": 4, "two_rounds": 8}          # the problem a round's end falls into
_CACHE = {}


@pytest.fixture(autouse=True)
def _release_allocations():
    yield
    torch.cuda.synchronize()
    del _ALIVE[:]


def ceil_div(a, b):
    return (a + b - 1) // b


def tiles_of(s):
    return ceil_div(s[1], 256) * ceil_div(s[2], 256)


def tile_coords(t, tiles_n, tiles_k, gm=4):
    """csrc/gemm.hip tile_coords: logical tile of a problem's grid -> (row tile, column tile)"""
    gsz = gm * tiles_k
    g = t // gsz
    first = g * gm
    rows = min(gm, tiles_n - first)
    r = t - g * gsz
    return first + r % rows, r // rows


@pytest.fixture
def sixteen_cus(lib):
    with tuned({5: 2, 12: lib.x2_device_cus() - CUS}):
        yield


def operands(name):
    """device operands (slices of NaN-filled buffers) and the float64 products of a queue, built once"""
    if name not in _CACHE:
        ops = []
        for i, (Mc, N, Kd) in enumerate(QUEUES[name]):
            dY, X = bf(rnd(Mc, N, seed=100 + i)), bf(rnd(Mc, Kd, seed=200 + i))
            ops.append((filled(dY, ld=N + 8), filled(X, ld=Kd + 8), dY.double().t() @ X.double()))
        _CACHE[name] = ops
    return _CACHE[name]


def run_queue(K, name, accumulate, ws_slices=4, via_wrapper=False):
    shapes = QUEUES[name]
    total = sum(tiles_of(s) for s in shapes)
    outs, guards, flat = [], [], []
    for (dY, X, _), (Mc, N, Kd) in zip(operands(name), shapes):
        dW, g = guarded((N, Kd), F32, ld=Kd + 4, name="dW")
        dW.fill_(1.5)
        outs.append(dW); guards.append(g)
        flat += [dY.data_ptr(), X.data_ptr(), dW.data_ptr(), Mc, N, Kd, dY.stride(0), X.stride(0), dW.stride(0), N, Kd]
    if via_wrapper:
        order = []
        K.gemm_tn_queue([(o[0], o[1], dW, s[1], s[2]) for o, dW, s in zip(operands(name), outs, shapes)], accumulate=bool(accumulate),
                        done=order.append)
        assert order == list(range(len(shapes)))
    else:
        room = ws_slices * (total % CUS) * 65536
        ws, g = guarded((max(room, 1),), F32, tail=65536, name="ws")
        guards.append(g)
        K.call("x2_gemm_tn_queue", (C.c_int64 * len(flat))(*flat), len(shapes), accumulate, K.ptr(ws) if room else None, room, 0, 0)
    torch.cuda.synchronize()
    for g in guards:
        g()
    return outs


def alone_unsplit(K, name, accumulate):
    """every problem by itself through gemm_tn_grouped(split=1): the instructions an unsplit tile runs today"""
    outs = []
    for (dY, X, _), (Mc, N, Kd) in zip(operands(name), QUEUES[name]):
        dW = torch.full((N, Kd), 1.5, device="cuda")
        K.gemm_tn_grouped([(dY, X, dW, N, Kd)], accumulate=bool(accumulate), split=1)
        outs.append(dW)
    return outs


@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("name", sorted(QUEUES))
def test_queue_against_float64_and_unsplit_launches(K, sixteen_cus, name, accumulate):
    shapes = QUEUES[name]
    windows, launches = K.tn_plan(shapes, cus=0, ws_floats=4 * CUS * 65536)
    assert [sp for sp, rem in launches if rem] == [WANT_SPLIT[name]] and all(sp == 1 for sp, rem in launches if not rem)
    assert len({l for l, p, f, n in windows if p == CUT[name]}) == 2                                  # a problem finished by two launches
    assert [p for _, p, f, _ in windows if f > 0] == [CUT[name]]                                      # a window starting mid-problem
    got = run_queue(K, name, accumulate)
    again = run_queue(K, name, accumulate)
    alone = alone_unsplit(K, name, accumulate)
    for i, ((_, _, ref), s) in enumerate(zip(operands(name), shapes)):
        err = relerr(got[i], ref + (1.5 if accumulate else 0.0))
        print(name, "problem", i, s, "relerr %.3g" % err)
        assert err < 1e-5, (name, i, s)
        assert torch.equal(got[i].view(I32), again[i].view(I32)), (name, i, "two runs differ")
    for launch, prob, first, n in windows:
        if launches[launch][0] != 1:
            continue
        N, Kd = shapes[prob][1:]
        for t in range(first, first + n):
            tn, tk = tile_coords(t, ceil_div(N, 256), ceil_div(Kd, 256))
            a = got[prob][tn * 256:(tn + 1) * 256, tk * 256:(tk + 1) * 256]
            b = alone[prob][tn * 256:(tn + 1) * 256, tk * 256:(tk + 1) * 256]
            assert torch.equal(a.contiguous().view(I32), b.contiguous().view(I32)), (name, prob, t, "differs from gemm_tn_grouped(split=1)")


def test_queue_without_workspace_never_splits(K, sixteen_cus):
    """ws = NULL: the remainder of the split-2 queue runs unsplit and every tile is gemm_tn_grouped(split=1)'s"""
    got = run_queue(K, "split2", 0, ws_slices=0)
    alone = alone_unsplit(K, "split2", 0)
    for a, b in zip(got, alone):
        assert torch.equal(a.contiguous().view(I32), b.view(I32))


@pytest.mark.parametrize("name", ["nine_problems", "split3"])
def test_wrapper_runs_the_plan_a_launch_at_a_time(K, sixteen_cus, name):
    """kernels.gemm_tn_queue(done=...): one x2_gemm_tn_queue call per launch of the plan, done(i) in problem order; the same integers as the
    whole plan in one call"""
    whole = run_queue(K, name, 0)
    stepped = run_queue(K, name, 0, via_wrapper=True)
    for a, b in zip(whole, stepped):
        assert torch.equal(a.contiguous().view(I32), b.contiguous().view(I32))


def test_queue_of_one_round_is_the_grouped_launch(K, lib):
    """no reservation, automatic kernel choice: 25 tiles fit one round and run as ONE launch of 9 entries (beyond the grouped entry's limit
    of 8) - held to float64 and to the sentinels"""
    got = run_queue(K, "nine_problems", 0)
    for i, (_, _, ref) in enumerate(operands("nine_problems")):
        assert relerr(got[i], ref) < 1e-5, i
