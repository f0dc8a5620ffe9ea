"""The retrieval kernels (csrc/retrieval.hip) against float64 restatements of the reference's expressions.

Soft-label ITC (x2_itc_soft_fwd / _bwd) against float64 torch autograd of xvlm.py:817-826:
    pos = idx == idx^T, lab = pos / pos.sum(1), (mean_i -sum(log_softmax(z, 1) lab) + mean_j -sum(log_softmax(z^T, 1) lab)) / 2.
Metric and bound: relerr and slice_relerr (row by row) at 1e-5 of max-abs, the project's fp32 rule (tests/test_cls_kernels_gpu.py), for the loss,
the 2N per-row / per-column losses, lse (the sum of the statistics' two parts) and dlogits; counts must be exact.
  N in {2, 3, 63, 64, 65, 257, 1024}: the smallest call; around one wave and one 64-column workgroup; past one 256-thread trip; the bound.
  ld = ldd = N, and N + 4 with NaN in the pad columns of the logits and sentinels in those of dlogits.
  idx: all distinct (must also equal ops.cross_entropy with arange labels in both directions: each side is within 1e-5 of float64, so they are
  within 2e-5 of each other), adjacent pairs, one group holding rows 63 and 64 (a wave boundary; rows 0 and N - 1 where N < 65), one group of all.
  logits at scale 14 (unit features over temp 0.07) and one case drawn from +-1000 (temp clamped to 0.001); g = 1 and 0.37.
Every output is written inside kernel_helpers.guarded sentinels and a second run gives the same bits.

x2_sample_negatives_checked against x2_sample_negatives on identical inputs: the same out, bit for bit, with and without groups, flags all 0;
ids all equal: flags all 1 and out[b] == b.  Group ids are an equivalence, so ids alone flag either no row or every row; the one way a single row
has no candidate is a row of similarities without a positive weight - NaN similarities - and that row alone is flagged.

x2_retrieval_ranks against cases_retrieval.ranks_float64, the declared rule restated in numpy (the number of STRICTLY greater scores, least over
the row's ground truths), for (R, N) in {(1, 1), (5, 10), (65, 37), (3, 257), (2, 4097), (2, 25010)}: the smallest call, fewer columns than
threads, more rows than a wave, past one trip, N past 4096 and COCO's 25 010 captions; ld = N and N + 3 with NaN pads; one ground truth per row,
five, ragged including none; ids -1 and N (skipped); -100 fill outside a top 12; counts over two calls; and, on tie-free matrices, np.argsort."""
import importlib

import numpy as np
import pytest
import torch

from cases_retrieval import ranks_float64
from kernel_helpers import F32, I32, I64, K, filled, guarded, relerr, slice_relerr  # noqa: F401  (K: fixture)

pytestmark = pytest.mark.gpu
dev = "cuda"
TOL = 1e-5
INT_MAX = 2 ** 31 - 1


def _call(name, *args):
    lib = importlib.import_module("x2-vlm_amd._lib")
    lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def check(name, got, ref, tol=TOL):
    ref = ref.reshape(got.shape)
    whole = relerr(got, ref)
    sl = slice_relerr(got, ref) if got.dim() == 2 else whole
    print("%-64s relerr %.3e  slice_relerr %.3e  (bound %.0e)" % (name, whole, sl, tol))
    assert whole < tol and sl < tol, (name, whole, sl, tol)


# ---------------------------------------------------------------------------------------------------- soft-label ITC

def idx_pattern(kind, N):
    g = torch.Generator().manual_seed(N)
    if kind == "distinct":
        return torch.randperm(N, generator=g) * 7 + 3
    if kind == "pairs":
        return torch.arange(N) // 2 + 100
    if kind == "boundary":
        idx = torch.arange(N) * 3 + 1
        a, b = (63, 64) if N > 64 else (0, N - 1)
        idx[b] = idx[a]
        return idx
    return torch.full((N,), 42, dtype=torch.int64)


def reference(z, idx, g):
    z = z.double().requires_grad_()
    pos = (idx.view(-1, 1) == idx.view(1, -1)).double()
    lab = pos / pos.sum(1, keepdim=True)
    li = -(torch.log_softmax(z, dim=1) * lab).sum(1)
    lt = -(torch.log_softmax(z.t(), dim=1) * lab).sum(1)
    loss = (li.mean() + lt.mean()) / 2
    (dz,) = torch.autograd.grad(loss * g, z)
    return dict(loss=loss.detach().reshape(1), rows=torch.cat([li, lt]).detach(), dz=dz, cnt=pos.sum(1),
                lse_r=torch.logsumexp(z.detach(), 1), lse_c=torch.logsumexp(z.detach(), 0))


def run_itc(z, idx, g, pad):
    N = z.shape[0]
    zd = filled(z, ld=N + pad)                                   # pad columns: NaN
    idxd = filled(idx)
    rowstat, g_rs = guarded((N, 3), F32, name="rowstat")
    colstat, g_cs = guarded((N, 3), F32, name="colstat")
    rows, g_rows = guarded((2 * N,), F32, name="loss_rows")
    out, g_out = guarded((1,), F32, name="out")
    dz, g_dz = guarded((N, N), F32, ld=N + pad, name="dlogits")
    gd = filled(torch.tensor([g], dtype=F32))
    res = []
    for _ in range(2):                                           # the second run: the same bits
        _call("x2_itc_soft_fwd", zd, N + pad, idxd, N, rowstat, colstat, rows, out)
        _call("x2_itc_soft_bwd", zd, N + pad, idxd, N, rowstat, colstat, gd, dz, N + pad)
        torch.cuda.synchronize()
        res.append([t.clone() for t in (rowstat, colstat, rows, out, dz)])
    for a, b in zip(*res):
        assert torch.equal(a, b)
    for gd_ in (g_rs, g_cs, g_rows, g_out, g_dz):
        gd_()
    return res[0]


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 257, 1024])
def test_itc_soft_against_float64(N, pad):
    ops = importlib.import_module("x2-vlm_amd.ops")
    gen = torch.Generator().manual_seed(31 * N + pad)
    fi = torch.nn.functional.normalize(torch.randn(N, 32, generator=gen), dim=1)
    ft = torch.nn.functional.normalize(torch.randn(N, 32, generator=gen), dim=1)
    z = (fi @ ft.t() / 0.07).float().contiguous()                # |z| <= 14.3
    for kind in ("distinct", "pairs", "boundary", "all"):
        idx = idx_pattern(kind, N)
        for g in (1.0, 0.37):
            ref = reference(z, idx, g)
            rowstat, colstat, rows, out, dz = run_itc(z, idx, g, pad)
            tag = "itc N=%d pad=%d %s g=%.2f: " % (N, pad, kind, g)
            check(tag + "loss", out, ref["loss"])
            check(tag + "li / lt", rows, ref["rows"])
            check(tag + "row lse", rowstat[:, 0].double() + rowstat[:, 1].double(), ref["lse_r"])
            check(tag + "column lse", colstat[:, 0].double() + colstat[:, 1].double(), ref["lse_c"])
            check(tag + "dlogits", dz, ref["dz"])
            assert torch.equal(rowstat[:, 2].cpu().double(), ref["cnt"]) and torch.equal(colstat[:, 2].cpu().double(), ref["cnt"])
        if kind == "distinct":
            # the pre-training labels: ops.itc_soft must agree with the two cross-entropies it generalises, value and gradient
            za, zb = z.to(dev).requires_grad_(), z.to(dev).requires_grad_()
            ar = torch.arange(N, device=dev)
            la = ops.itc_soft(za, idx.to(dev))
            lb = (ops.cross_entropy(zb, ar) + ops.cross_entropy(zb.t(), ar)) / 2
            (la * 0.37).backward()
            (lb * 0.37).backward()
            e_l, e_g = relerr(la.detach().reshape(1), lb.detach().cpu().reshape(1)), relerr(za.grad, zb.grad.cpu())
            print("itc N=%d distinct: ops.itc_soft vs 2 x ops.cross_entropy: loss %.3e, gradient %.3e (bound %.0e)" % (N, e_l, e_g, 2 * TOL))
            assert e_l < 2 * TOL and e_g < 2 * TOL
            check("itc N=%d distinct: ops.itc_soft" % N, la.detach().reshape(1), reference(z, idx, 1.0)["loss"])


def test_itc_soft_at_the_clamped_temperature():
    """temp clamped to 0.001: logits of +-1000.  lse is kept as {max, log-sum} so that exp(z - lse) does not inherit the 6e-5 spacing of an fp32
    number near 1000."""
    N = 65
    gen = torch.Generator().manual_seed(5)
    z = ((torch.rand(N, N, generator=gen) * 2 - 1) * 1000.0).float()
    z[torch.arange(N), torch.arange(N)] += 3.0                   # a few rows whose positive is (close to) the maximum
    for kind in ("pairs", "all"):
        idx = idx_pattern(kind, N)
        ref = reference(z, idx, 1.0)
        rowstat, colstat, rows, out, dz = run_itc(z, idx, 1.0, 4)
        check("itc +-1000 %s: loss" % kind, out, ref["loss"])
        check("itc +-1000 %s: li / lt" % kind, rows, ref["rows"])
        check("itc +-1000 %s: dlogits" % kind, dz, ref["dz"])
        assert bool(torch.isfinite(dz).all())


def test_itc_soft_through_autograd_on_a_strided_view():
    """ops.itc_soft on a row-padded view (stride N + 4, NaN pads), g arriving from autograd (the captured step: tests/test_retrieval_step_gpu.py)"""
    ops = importlib.import_module("x2-vlm_amd.ops")
    N = 65
    gen = torch.Generator().manual_seed(9)
    z = (torch.randn(N, N, generator=gen) * 5).float()
    idx = idx_pattern("pairs", N)
    ref = reference(z, idx, 0.37)
    base = torch.full((N, N + 4), float("nan"), device=dev)
    base[:, :N] = z.to(dev)
    leaf = base.requires_grad_()
    loss = ops.itc_soft(leaf[:, :N], idx.to(dev))
    (loss * 0.37).backward()
    check("ops.itc_soft strided: loss", loss.detach().reshape(1), ref["loss"])
    check("ops.itc_soft strided: dlogits", leaf.grad[:, :N], ref["dz"])


# ---------------------------------------------------------------------------------------------------- the checked sampler

@pytest.mark.parametrize("n", [2, 5, 65, 1024])
def test_checked_sampler_is_the_sampler_plus_flags(K, n):
    gen = torch.Generator().manual_seed(n)
    sim = (torch.randn(n, n, generator=gen) * 3).to(dev)
    u = torch.rand(n, generator=gen).to(dev)
    groups = [None, (torch.arange(n) // 2 + 7).to(dev)] if n > 2 else [None]
    for grp in groups:
        want = K.sample_negatives(sim, u, grp)
        out, flags = guarded((n,), I32, name="out"), guarded((n,), I32, name="no_negative")
        _call("x2_sample_negatives_checked", sim, n, grp if grp is not None else None, u, out[0], flags[0])
        torch.cuda.synchronize()
        out[1](), flags[1]()
        assert torch.equal(out[0], want), (n, grp is not None)
        assert not bool(flags[0].any())
        got, fl = K.sample_negatives_checked(sim, u, grp)
        assert torch.equal(got, want) and not bool(fl.any()) and got.dtype == torch.int32 and fl.dtype == torch.int32
        same = want.long().cpu() == torch.arange(n)
        assert not bool(same.any())
        if grp is not None:
            assert not bool((grp.cpu()[want.long().cpu()] == grp.cpu()).any())
    # every id equal: no row has a negative; the in-range fallback
    one = torch.full((n,), 5, dtype=I64, device=dev)
    got, fl = K.sample_negatives_checked(sim, u, one)
    assert torch.equal(fl.cpu(), torch.ones(n, dtype=I32)) and torch.equal(got.cpu(), torch.arange(n, dtype=I32))
    assert torch.equal(K.sample_negatives(sim, u, one), got)
    # exactly one row without a candidate of positive weight (ids are an equivalence: they flag no row or all of them)
    if n > 2:
        b = n // 2
        bad = sim.clone()
        bad[b] = float("nan")
        got, fl = K.sample_negatives_checked(bad, u, groups[-1])
        want_flags = torch.zeros(n, dtype=I32)
        want_flags[b] = 1
        assert torch.equal(fl.cpu(), want_flags) and int(got[b]) == b
        keep = torch.arange(n) != b
        assert torch.equal(got.cpu()[keep], K.sample_negatives(sim, u, groups[-1]).cpu()[keep])


# ---------------------------------------------------------------------------------------------------- ranks and recall counts

def ground_truths(mode, R, N, gen):
    if mode == "one":
        return [[int(torch.randint(0, N, (1,), generator=gen))] for _ in range(R)]
    if mode == "five":
        return [torch.randint(0, N, (5,), generator=gen).tolist() for _ in range(R)]
    if mode == "ragged":                                          # 0, 1, 2, ... 9 ground truths, more than one pass of eight, row 0 none
        return [torch.randint(0, N, (r % 10,), generator=gen).tolist() for r in range(R)]
    gt = [torch.randint(0, N, (3,), generator=gen).tolist() for _ in range(R)]      # "skipped": ids -1 and N among (or instead of) the valid ones
    for r in range(R):
        gt[r][r % 3] = -1 if r % 2 else N
    gt[R - 1] = [-1, N]
    return gt


def csr(gt):
    offs = np.cumsum([0] + [len(g) for g in gt]).astype(np.int32)
    ids = np.array([j for g in gt for j in g], dtype=np.int32)
    return torch.from_numpy(offs), torch.from_numpy(ids)


def counts_of(ranks):
    return [int((ranks < k).sum()) for k in (1, 5, 10)] + [len(ranks)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("R,N", [(1, 1), (5, 10), (65, 37), (3, 257), (2, 4097), (2, 25010)])
def test_retrieval_ranks_against_the_declared_rule(K, R, N, pad):
    gen = torch.Generator().manual_seed(1000 * R + N)
    dense = torch.randn(R, N, generator=gen)
    mats = {"dense": dense}
    if N > 12:
        fill = torch.full((R, N), -100.0)
        top = dense.topk(12, dim=1).indices
        mats["top12"] = fill.scatter(1, top, dense.gather(1, top))
    total = np.zeros(4, dtype=np.int64)
    counts, g_counts = guarded((4,), I64, name="counts")
    counts.zero_()
    for mname, m in mats.items():
        md = filled(m, ld=N + pad)
        for mode in ("one", "five", "ragged", "skipped"):
            gt = ground_truths(mode, R, N, gen)
            offs, ids = csr(gt)
            want = ranks_float64(m.numpy(), gt)
            ranks, g_ranks = guarded((R,), I32, name="ranks")
            before = counts.clone()
            _call("x2_retrieval_ranks", md, N + pad, R, N, filled(offs), filled(ids) if ids.numel() else 0, ranks, counts)
            torch.cuda.synchronize()
            g_ranks(), g_counts()
            assert np.array_equal(ranks.cpu().numpy().astype(np.int64), want), (mname, mode)
            total += np.array(counts_of(want))
            assert (counts - before).cpu().tolist() == counts_of(want)          # counts accumulate over the calls
            if mode == "skipped":
                assert want[R - 1] == INT_MAX
    assert counts.cpu().tolist() == total.tolist() and total[3] == R * 4 * len(mats)
    # the wrapper on a view with a row stride
    gt = ground_truths("ragged", R, N, gen)
    offs, ids = csr(gt)
    c2 = torch.zeros(4, dtype=I64, device=dev)
    wide = torch.full((R, N + 5), float("nan"), device=dev)
    wide[:, :N] = dense.to(dev)
    ranks = K.retrieval_ranks(wide[:, :N], offs.to(dev), ids.to(dev), c2)
    K.retrieval_ranks(wide[:, :N], offs.to(dev), ids.to(dev), c2)
    want = ranks_float64(dense.numpy(), gt)
    assert np.array_equal(ranks.cpu().numpy().astype(np.int64), want) and c2.cpu().tolist() == [2 * v for v in counts_of(want)]


@pytest.mark.parametrize("R,N", [(5, 10), (65, 37), (2, 25010)])
def test_retrieval_ranks_equal_argsort_without_ties(K, R, N):
    """On a matrix without equal scores the declared rule IS itm_eval's: np.where(np.argsort(score)[::-1] == i)"""
    gen = torch.Generator().manual_seed(R + N)
    m = torch.stack([torch.randperm(N, generator=gen) for _ in range(R)]).float() * 0.25 - 3.0       # distinct, exact in fp32
    gt = [torch.randint(0, N, (1 + r % 4,), generator=gen).tolist() for r in range(R)]
    offs, ids = csr(gt)
    counts = torch.zeros(4, dtype=I64, device=dev)
    ranks = K.retrieval_ranks(m.to(dev), offs.to(dev), ids.to(dev), counts).cpu().numpy()
    want = []
    for r in range(R):
        inds = np.argsort(m[r].numpy())[::-1]
        want.append(min(int(np.where(inds == i)[0][0]) for i in gt[r]))
    assert ranks.tolist() == want and counts.cpu().tolist() == counts_of(np.array(want))


def test_retrieval_eval_figures(K):
    """retrieval_eval: the reference's nine keys from two device matrices, an image without captions in the denominator"""
    mr = importlib.import_module("x2-vlm_amd.model_retrieval")
    from cases_retrieval import recall_from_ranks
    gen = torch.Generator().manual_seed(77)
    Ni, Nt = 7, 23
    i2t, t2i = torch.randn(Ni, Nt, generator=gen), torch.randn(Nt, Ni, generator=gen)
    img2txt = {i: list(range(4 * i, min(Nt, 4 * i + 4))) for i in range(Ni) if i != 2}            # image 2: no caption
    txt2img = [min(j // 4, Ni - 1) for j in range(Nt)]
    got = mr.retrieval_eval(i2t.to(dev), t2i.to(dev), txt2img, img2txt)
    want = recall_from_ranks(ranks_float64(i2t.numpy(), [img2txt.get(i, []) for i in range(Ni)]), ranks_float64(t2i.numpy(), [[j] for j in txt2img]))
    assert list(got) == list(mr.RECALL_KEYS) and got == want
    assert got["txt_r10"] <= 100.0 * (Ni - 1) / Ni
