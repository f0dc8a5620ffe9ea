"""The grounding kernels (csrc/grounding.hip) against float64 autograd of the reference's expressions, restated here: XVLMBase.get_bbox_loss
with box_ops.py (xvlm.py:927-957: sigmoid, L1, 1 - GIoU of matched pairs through cx +- w / 2, the any-degenerate early-out, the keep-weighted
means) and grounding_eval_bbox / computeIoU (dataset/utils.py:363-453; cases_grounding.iou_float64).

Shapes: B in {1, 2, 63, 64, 65, 256, 257, 1025} - one row, a partial wave, one short of / at / one past a wave and the 256-thread workgroup
(the forward's stride, the backward's grid), five trips of the forward's row loop - with keep NULL, mixed and a single kept row.  Metric and
bound: relerr and slice_relerr (row by row) at 1e-5 of max-abs, the project's fp32 rule (tests/test_small_kernels_gpu.py).  Inputs: logits in
[-4, 4]; every quantity that passes through max / min / abs / clamp at least 1e-3 from its kink in float64 (rows are redrawn until it holds),
so the kernel's documented tie choices are never exercised.  Measured worst: coord 9.9e-8, the two means 1.5e-7, dlogits 3.4e-6 on
overlapping boxes and 7.8e-6 on nested ones (a prediction 0.02 wide whose edges come from cx +- w / 2, the reference's own route: the fp32
rounding of an edge near 0.5 is 3e-6 of such a width).  Every output and `stat` is written inside kernel_helpers.guarded sentinels.

x2_grounding_iou: N in {1, 255, 256, 257, 5000}; the set starts with constructed rows (touching edges, a box inside the other, disjoint boxes,
an exact match).  IoU bound 1e-5 absolute: pixel coordinates below 1024 carry fp32 rounding errors of at most 2^-14 = 6e-5 px per operation,
a handful of operations deep, on extents of at least 0.15 x 240 = 36 px, so an area ratio moves by a few 1e-6 (the reference's own mixed
fp32 / float64 evaluation is 5.9e-7 from the float64 restatement on the golden set: tests/golden/make_golden_grounding.py).  `hit` is compared
wherever the float64 IoU is more than 1e-4 from 0.5; at least 95 % of the seeded rows must be (checked here and when the seed was chosen)."""
import importlib

import numpy as np
import pytest
import torch

from cases_grounding import eval_set, iou_float64, kink_margin
from kernel_helpers import F32, I32, K, filled, guarded, relerr, slice_relerr  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
dev = "cuda"
TOL = 1e-5
KINK = 1e-3
SIZES = [1, 2, 63, 64, 65, 256, 257, 1025]
COTANGENTS = [(1.0, 1.0, False), (0.3, 0.0, False), (0.0, 2.0, False), (1.0, 1.0, True)]


def _call(name, *args):
    lib = importlib.import_module("x2-vlm_amd._lib")
    lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def check(name, got, ref, tol=TOL):
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    whole, sl = relerr(got, ref), slice_relerr(got, ref)
    print("%-52s relerr %.3e  slice_relerr %.3e  (bound %.0e)" % (name, whole, sl, tol))
    assert whole < tol and sl < tol, (name, whole, sl, tol)


def row_margin(coord, target):
    return np.array([kink_margin(coord[i:i + 1], target[i:i + 1]) for i in range(coord.shape[0])])


def draw(B, seed, geometry="mixed"):
    """(logits, target) fp32 [B, 4] with every row at least KINK from every kink.  geometry: 'mixed' (overlapping, as drawn), 'disjoint' (the
    target beside the prediction: zero intersection), 'nested' (alternately the target inside the prediction and around it)."""
    r = np.random.default_rng([seed, B])
    logits, target = np.zeros((B, 4), np.float32), np.zeros((B, 4), np.float32)
    todo = np.arange(B)
    for _ in range(64):
        n = len(todo)
        z = r.uniform(-4.0, 4.0, size=(n, 4)).astype(np.float32)
        c = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
        if geometry == "mixed":
            wh = r.uniform(0.1, 0.7, size=(n, 2))
            t = np.concatenate([r.uniform(0.0, 1.0, size=(n, 2)) * (1 - wh) + wh / 2, wh], axis=1)
        elif geometry == "disjoint":
            wh = r.uniform(0.1, 0.5, size=(n, 2))
            gap = r.uniform(0.01, 0.3, size=n)
            side = r.integers(0, 2, size=n) * 2 - 1
            t = np.concatenate([c[:, :2] + r.uniform(-0.2, 0.2, size=(n, 2)), wh], axis=1)
            t[:, 0] = c[:, 0] + side * (c[:, 2] / 2 + wh[:, 0] / 2 + gap)          # beside the prediction along x
        else:
            f = np.where((np.arange(n) % 2 == 0)[:, None], r.uniform(0.3, 0.8, size=(n, 2)), r.uniform(1.3, 2.5, size=(n, 2)))
            wh = c[:, 2:] * f
            room = np.abs(c[:, 2:] - wh) / 2
            t = np.concatenate([c[:, :2] + r.uniform(-0.8, 0.8, size=(n, 2)) * room, wh], axis=1)
        t = t.astype(np.float32)
        ok = row_margin(c, t) >= KINK
        logits[todo[ok]], target[todo[ok]] = z[ok], t[ok]
        todo = todo[~ok]
        if len(todo) == 0:
            break
    assert len(todo) == 0
    return torch.from_numpy(logits), torch.from_numpy(target)


def keep_of(mode, B, seed):
    if mode == "none":
        return None
    k = torch.zeros(B)
    if mode == "mixed":
        k = (torch.rand(B, generator=torch.Generator().manual_seed(seed)) < 0.6).float()
        k[B // 2] = 1.0
        if B > 1:
            k[(B // 2 + 1) % B] = 0.0
    else:
        k[(2 * B) // 3] = 1.0
    return k


def xyxy(b):
    cx, cy, w, h = b.unbind(-1)
    return torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)


def reference(logits, target, keep, g_bbox=1.0, g_giou=1.0, g_coord=None):
    """float64 autograd of xvlm.py:923, 927-957 with box_ops.generalized_box_iou's diagonal -> coord, loss_bbox, loss_giou, flag, num, dlogits"""
    z = logits.double().requires_grad_(True)
    t = target.double()
    c = z.sigmoid()
    l1 = (c - t).abs()
    a, b = xyxy(c), xyxy(t)
    flag = bool((a[:, 2:] < a[:, :2]).any() or (b[:, 2:] < b[:, :2]).any())
    if flag:
        giou = torch.zeros(c.shape[0], dtype=torch.float64)
    else:
        area1, area2 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
        inter = wh[:, 0] * wh[:, 1]
        union = area1 + area2 - inter
        whc = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
        area = whc[:, 0] * whc[:, 1]
        giou = 1 - (inter / union - (area - union) / area)
    if keep is None:
        num = float(c.shape[0])
    else:
        k = keep.double()
        num = float(k.sum())
        l1, giou = l1 * k.view(-1, 1), giou * k
    loss_bbox, loss_giou = l1.sum() / num, giou.sum() / num
    total = g_bbox * loss_bbox + g_giou * loss_giou
    if g_coord is not None:
        total = total + (g_coord.double() * c).sum()
    total.backward()
    return c.detach(), float(loss_bbox.detach()), float(loss_giou.detach()), flag, num, z.grad


def run_forward(logits, target, keep):
    """x2_bbox_loss_fwd into guarded outputs, inputs in guarded copies -> (coord, stat, device inputs)"""
    B = logits.shape[0]
    zl, tg = filled(logits), filled(target)
    kp = None if keep is None else filled(keep)
    coord, g_c = guarded((B, 4), F32, name="coord")
    stat, g_s = guarded((4,), F32, name="stat")
    _call("x2_bbox_loss_fwd", zl, tg, kp, B, coord, stat)
    torch.cuda.synchronize()
    g_c(), g_s()
    return coord, stat, (zl, tg, kp)


def run_backward(coord, tg, kp, stat, g_bbox, g_giou, g_coord):
    B = coord.shape[0]
    gb = None if g_bbox is None else filled(torch.tensor([g_bbox]))
    gg = None if g_giou is None else filled(torch.tensor([g_giou]))
    gc = None if g_coord is None else filled(g_coord)
    dl, g_d = guarded((B, 4), F32, name="dlogits")
    _call("x2_bbox_loss_bwd", coord, tg, kp, stat, gb, gg, gc, B, dl)
    torch.cuda.synchronize()
    g_d()
    return dl


def check_stat(name, stat, lb, lg, flag, num):
    s = stat.cpu().double()
    print("%-52s loss_bbox %.3e  loss_giou %.3e" % (name + " stat", abs(float(s[0]) - lb) / max(abs(lb), 1e-12), abs(float(s[1]) - lg) / max(abs(lg), 1e-12) if lg else abs(float(s[1]))))
    assert abs(float(s[0]) - lb) < TOL * abs(lb)
    assert (float(s[1]) == 0.0) if flag else abs(float(s[1]) - lg) < TOL * abs(lg)
    assert float(s[2]) == (1.0 if flag else 0.0) and float(s[3]) == num


@pytest.mark.parametrize("mode", ["none", "mixed", "single"])
@pytest.mark.parametrize("B", SIZES)
def test_bbox_loss_forward_backward(K, B, mode):
    logits, target = draw(B, 1)
    keep = keep_of(mode, B, 5)
    coord, stat, (zl, tg, kp) = run_forward(logits, target, keep)
    g_coord = torch.randn(B, 4, generator=torch.Generator().manual_seed(9)) * 0.5
    name = "B=%d keep=%s" % (B, mode)
    for g_bbox, g_giou, with_coord in COTANGENTS:
        c, lb, lg, flag, num, dz = reference(logits, target, keep, g_bbox, g_giou, g_coord if with_coord else None)
        assert not flag
        dl = run_backward(coord, tg, kp, stat, g_bbox, g_giou, g_coord if with_coord else None)
        check("%s dlogits cot=(%g, %g%s)" % (name, g_bbox, g_giou, ", g_coord" if with_coord else ""), dl, dz)
    check(name + " coord", coord, c)
    check_stat(name, stat, lb, lg, False, num)
    # a NULL cotangent is a zero cotangent
    assert torch.equal(run_backward(coord, tg, kp, stat, None, 2.0, None), run_backward(coord, tg, kp, stat, 0.0, 2.0, None))
    assert torch.equal(run_backward(coord, tg, kp, stat, 0.3, None, None), run_backward(coord, tg, kp, stat, 0.3, 0.0, None))
    # two runs give the same bits (one workgroup, fixed order, no atomics)
    coord2, stat2, _ = run_forward(logits, target, keep)
    assert torch.equal(coord, coord2) and torch.equal(stat, stat2)
    assert torch.equal(run_backward(coord, tg, kp, stat, 1.0, 1.0, g_coord), run_backward(coord2, tg, kp, stat2, 1.0, 1.0, g_coord))
    # the tensor-level wrappers and the autograd function launch the same kernels
    ops = importlib.import_module("x2-vlm_amd.ops")
    zt = logits.to(dev).requires_grad_(True)
    is_image = None if keep is None else (1 - keep).to(dev)
    oc, ob, og = ops.bbox_loss(zt, target.to(dev), is_image)
    (ob + og + (oc * g_coord.to(dev)).sum()).backward()
    assert torch.equal(oc.detach(), coord) and float(ob.detach()) == float(stat[0]) and float(og.detach()) == float(stat[1])
    assert torch.equal(zt.grad, run_backward(coord, tg, kp, stat, 1.0, 1.0, g_coord))


@pytest.mark.parametrize("geometry", ["disjoint", "nested"])
@pytest.mark.parametrize("B", [2, 65, 257])
def test_bbox_loss_box_geometry(K, B, geometry):
    logits, target = draw(B, 2, geometry)
    c64 = torch.sigmoid(logits.double())
    a, b = xyxy(c64), xyxy(target.double())
    overlap = torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])
    if geometry == "disjoint":
        assert bool((overlap[:, 0] < 0).all())                                        # zero intersection in every row
    else:
        inside = ((b[:, :2] > a[:, :2]) & (b[:, 2:] < a[:, 2:])).all(1)
        around = ((b[:, :2] < a[:, :2]) & (b[:, 2:] > a[:, 2:])).all(1)
        assert bool((inside | around).all()) and bool(inside.any()) and bool(around.any())
    coord, stat, (zl, tg, kp) = run_forward(logits, target, None)
    c, lb, lg, flag, num, dz = reference(logits, target, None)
    assert not flag
    name = "B=%d %s" % (B, geometry)
    check(name + " coord", coord, c)
    check_stat(name, stat, lb, lg, False, num)
    check(name + " dlogits", run_backward(coord, tg, kp, stat, 1.0, 1.0, None), dz)
    _, _, _, _, _, dz_g = reference(logits, target, None, 0.0, 1.0)
    check(name + " dlogits, GIoU alone", run_backward(coord, tg, kp, stat, None, 1.0, None), dz_g)


@pytest.mark.parametrize("where", ["first", "last", "dropped"])
@pytest.mark.parametrize("B", [2, 65, 1025])
def test_bbox_loss_degenerate_rows(K, B, where):
    """a target of negative width in the first row, the last row, or a row with keep == 0: the flag is set, every row's GIoU term is 0 and
    gives no gradient; nothing is NaN although the flagged row's own GIoU expression is 0 / 0-free garbage"""
    logits, target = draw(B, 3)
    keep = None
    row = {"first": 0, "last": B - 1, "dropped": B // 2}[where]
    if where == "dropped":
        keep = torch.ones(B)
        keep[row] = 0.0
    target[row, 2] = -0.3
    target[(row + 1) % B, 2:] = 0.0                                                   # and a zero-area target elsewhere (not degenerate by itself)
    coord, stat, (zl, tg, kp) = run_forward(logits, target, keep)
    c, lb, lg, flag, num, dz = reference(logits, target, keep, 1.0, 1.0)
    assert flag and lg == 0.0
    name = "B=%d degenerate %s" % (B, where)
    check(name + " coord", coord, c)
    check_stat(name, stat, lb, lg, True, num)
    dl = run_backward(coord, tg, kp, stat, 1.0, 1.0, None)
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(stat).all())
    check(name + " dlogits", dl, dz)
    assert torch.equal(dl, run_backward(coord, tg, kp, stat, 1.0, None, None))      # exactly the L1 gradient
    assert float(run_backward(coord, tg, kp, stat, None, 1.0, None).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- evaluation

def iou_set(n):
    """n samples: constructed rows first (512 x 512 images: every normalised coordinate is exact in fp32), the rest cases_grounding.eval_set(seed 11)"""
    W, H = 512.0, 512.0
    rows = [  # (pred pixel xywh, ref pixel xywh)
        ((100, 100, 200, 100), (100, 100, 200, 100)),          # the same box: (w - 1 + 1) * (h - 1 + 1) over w * h
        ((100, 100, 100, 100), (200, 120, 100, 60)),           # touching along x: inclusive edges leave x1 = 200 > x2 = 199
        ((100, 100, 101, 100), (200, 120, 100, 60)),           # one pixel further: x1 = 200 == x2 = 200, the strict < says no overlap
        ((100, 100, 102, 100), (200, 120, 100, 60)),           # two pixels: overlaps
        ((50, 50, 400, 300), (150, 100, 100, 120)),            # the reference box inside the prediction
        ((200, 150, 60, 40), (100, 100, 300, 200)),            # the prediction inside the reference box
        ((20, 20, 100, 100), (350, 300, 150, 120)),            # disjoint
        ((20, 300, 100, 100), (30, 20, 150, 120)),             # disjoint along y only
    ][:n]
    pp = np.array([r[0] for r in rows], dtype=np.float64).reshape(-1, 4)
    pred = np.stack([(pp[:, 0] + pp[:, 2] / 2) / W, (pp[:, 1] + pp[:, 3] / 2) / H, pp[:, 2] / W, pp[:, 3] / H], axis=1).astype(np.float32)
    ref = np.array([r[1] for r in rows], dtype=np.float32).reshape(-1, 4)
    size = np.tile(np.array([[W, H]], dtype=np.float32), (len(rows), 1))
    if n > len(rows):
        p2, r2, s2, _ = eval_set(seed=11, n=n - len(rows))
        pred, ref, size = np.concatenate([pred, p2]), np.concatenate([ref, r2]), np.concatenate([size, s2])
    return pred, ref, size


@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
def test_grounding_iou(K, N):
    pred, ref, size = iou_set(N)
    want = iou_float64(pred, ref, size)
    iou, g_i = guarded((N,), F32, name="iou")
    hit, g_h = guarded((N,), I32, name="hit")
    _call("x2_grounding_iou", filled(torch.from_numpy(pred)), filled(torch.from_numpy(ref)), filled(torch.from_numpy(size)), N, iou, hit)
    torch.cuda.synchronize()
    g_i(), g_h()
    got = iou.cpu().double().numpy()
    err = float(np.abs(got - want).max())
    sure = np.abs(want - 0.5) > 1e-4
    print("grounding_iou N=%d: worst |iou - float64| %.3e (bound 1e-5); %.1f %% of rows comparable for hit; %d hits" % (N, err, 100 * sure.mean(), int((want >= 0.5).sum())))
    assert np.isfinite(got).all() and err <= 1e-5
    h = hit.cpu().numpy()
    assert set(np.unique(h).tolist()) <= {0, 1} and np.array_equal(h == 1, got >= 0.5)
    assert np.array_equal(h[sure] == 1, want[sure] >= 0.5)
    if N >= 255:
        assert sure.mean() >= 0.95
        # the constructed rows: equal boxes, touching (none), equal edges (none by the strict <), overlapping, nested twice, disjoint twice
        assert abs(want[0] - 1.0) < 1e-4 and want[1] == 0 and want[2] == 0 and want[3] > 0 and want[6] == 0 and want[7] == 0
        assert abs(want[4] - 100 * 120 / (400 * 300.0)) < 1e-3 and abs(want[5] - 60 * 40 / (300 * 200.0)) < 1e-3
        assert got[1] == 0 and got[2] == 0 and got[3] > 0 and got[6] == 0 and got[7] == 0
    iou2, hit2 = K.grounding_iou(torch.from_numpy(pred).to(dev), torch.from_numpy(ref).to(dev), torch.from_numpy(size).to(dev))
    assert torch.equal(iou2, iou) and torch.equal(hit2, hit)
