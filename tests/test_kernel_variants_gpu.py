"""GPU parity of the launch variants that the dispatchers pick from the problem size, at the sizes where the training step picks
them: LayerNorm forward with several rows per wave, the LayerNorm backward's dropout masks, the deferred stage-2 reductions the
engine runs on its side stream, hard-negative sampling inside `idx` groups, the packed bias vectors and the fp32 column sums of the
head biases.

References are float64 on the CPU after the kernels' own input rounding (bf16 inputs rounded first), as in test_kernels_gpu.py;
where a kernel claims bit-identical outputs across its variants, the test asserts bit equality.  Besides the whole-tensor bound,
LayerNorm outputs are bounded row by row against each row's own reference max-abs (`rowerr`)."""
import pytest
import torch

from kernel_helpers import K, bf, relerr, rnd, rowerr, tuned  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
dev = "cuda"
EPS = 1e-6


def ln64(x, w, b, eps=EPS):
    """float64 LayerNorm: (y, mean, rstd)."""
    x = x.double()
    mu = x.mean(-1, keepdim=True)
    rs = torch.rsqrt(((x - mu) ** 2).mean(-1, keepdim=True) + eps)
    return (x - mu) * rs * w.double() + b.double(), mu.squeeze(-1), rs.squeeze(-1)


def ln_inputs(rows, D, period, seed):
    total = rows if period == 0 else rows // period * (period + 1)
    x = rnd(total, D, seed=seed, scale=2.0) + 0.5
    w, b = rnd(D, seed=seed + 1) * 0.1 + 1, rnd(D, seed=seed + 2) * 0.1
    sel = torch.arange(total) if period == 0 else torch.tensor([r + r // period + 1 for r in range(rows)])
    return total, x, w, b, sel


def element_index(sel, D):
    """flat element index (row of the full token tensor * D + column) that the kernels hash for their dropout masks"""
    return sel.to(torch.int64)[:, None] * D + torch.arange(D, dtype=torch.int64)[None, :]


# ------------------------------------------------------------------------------------------------ LayerNorm forward, rows per wave

@pytest.mark.parametrize("rows,period", [(8191, 0), (8192, 0), (42 * 196, 196)], ids=["8191", "8192", "8232p196"])
@pytest.mark.parametrize("D", [128, 512, 768, 1000, 1024, 2048], ids=["nv1", "nv2", "nv3", "nv4ragged", "nv4", "nv8"])
def test_layernorm_fwd_rows_per_wave(K, rows, period, D):
    """x2_tune(13, v): one row per wave (layernorm_fwd_kernel<NV>) and 2 / 4 rows per wave (layernorm_fwd_rows_kernel<NV, RPW>; D > 1024
    always takes one row) and the automatic choice (2 from 8192 rows on): same arithmetic, same summation order, so y (fp32, bf16),
    mean and rstd are bit-identical across the forms and match float64; 8191 rows leave the last wave of every RPW form partial.
    With output dropout, y = reference x K.dropout_keep(spec, element index) - the index the host mirror and the backward use."""
    total, x, w, b, sel = ln_inputs(rows, D, period, seed=D + rows)
    ref, mu, rs = ln64(x[sel], w, b)
    spec = K.dropout_spec(0.1, 1234 + D, 7)
    keep = K.dropout_keep(spec, element_index(sel, D)).double()
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    outs, drops = {}, {}
    for v in (1, 2, 4, 0):
        with tuned({13: v}):
            outs[v] = K.layernorm_fwd(xd, wd, bd, EPS, rows=rows, period=period, want_f32=True)
            drops[v] = K.layernorm_fwd(xd, wd, bd, EPS, rows=rows, period=period, want_f32=True, drop=spec)
    selg = sel.to(dev)
    for v in (2, 4, 0):
        for a_, b_ in zip(outs[v], outs[1]):
            a_, b_ = (a_[selg], b_[selg]) if a_.dim() == 2 else (a_, b_)      # rows the period skips are not written
            assert torch.equal(a_, b_), v
        for a_, b_ in zip(drops[v], drops[1]):
            a_, b_ = (a_[selg], b_[selg]) if a_.dim() == 2 else (a_, b_)
            assert torch.equal(a_, b_), v
    yb, yf, mean, rstd = outs[1]
    assert relerr(yf[selg], ref) < 1e-5 and rowerr(yf[selg], ref) < 1e-5
    assert relerr(yb[selg], ref) < 6e-3 and rowerr(yb[selg], ref) < 6e-3
    assert relerr(mean, mu) < 1e-5 and relerr(rstd, rs) < 1e-5
    yb, yf, mean2, rstd2 = drops[1]
    assert torch.equal(mean2, mean) and torch.equal(rstd2, rstd)
    want = ref * keep
    assert relerr(yf[selg], want) < 1e-5 and rowerr(yf[selg], want) < 1e-5
    assert relerr(yb[selg], want) < 6e-3 and rowerr(yb[selg], want) < 6e-3
    assert torch.equal((yf[selg] == 0).cpu(), keep == 0)


# ------------------------------------------------------------------------------------------------ LayerNorm backward with dropout

@pytest.mark.parametrize("rows,D,period", [(788, 768, 0), (4 * 196, 1024, 196), (300, 1000, 0), (33, 2048, 0)])
def test_layernorm_bwd_dropout_masks(K, rows, D, period):
    """drop_in: the forward dropped the LN output (BertEmbeddings), so the incoming gradient carries that mask - dx, dw, db of
    sum(LN(x) * keep * dy).  drop_out: the producing linear's output was dropped before the residual add, so the bf16 copy and the
    column sums dcol carry the mask and the fp32 dx does not (x2_layernorm_bwd excludes dres with an output mask)."""
    total, x, w, b, sel = ln_inputs(rows, D, period, seed=3 * D + rows)
    dy, dres = rnd(total, D, seed=11), rnd(total, D, seed=12)
    s_in, s_out = K.dropout_spec(0.1, 4321, 2), K.dropout_spec(0.15, 977, 9)
    idx = element_index(sel, D)
    k_in, k_out = K.dropout_keep(s_in, idx).double(), K.dropout_keep(s_out, idx).double()
    xd, wd, bd, dyd = x.to(dev), w.to(dev), b.to(dev), dy.to(dev)
    _, yf, mean, rstd = K.layernorm_fwd(xd, wd, bd, EPS, rows=rows, period=period, want_f32=True, want_bf16=False, drop=s_in)
    y_ref = ln64(x[sel], w, b)[0]
    assert relerr(yf[sel.to(dev)], y_ref * k_in) < 1e-5

    def grads(mask):
        xl, wl, bl = (t.double().requires_grad_(True) for t in (x[sel], w, b))
        (ln64(xl, wl, bl)[0] * mask * dy[sel].double()).sum().backward()
        return xl.grad, wl.grad, bl.grad

    gx, gw, gb = grads(k_in)
    dw, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    dx, _ = K.layernorm_bwd(dyd, xd, mean, rstd, wd, dw, db, dres=dres.to(dev), period=period, drop_in=s_in)
    want = gx + dres[sel].double()
    assert relerr(dx[sel.to(dev)], want) < 2e-5 and rowerr(dx[sel.to(dev)], want) < 2e-5
    assert relerr(dw, gw) < 2e-5 and relerr(db, gb) < 2e-5
    gx, gw, gb = grads(1.0)
    dw, db, dcol = torch.zeros(D, device=dev), torch.zeros(D, device=dev), torch.zeros(D, device=dev)
    dx, dxb = K.layernorm_bwd(dyd, xd, mean, rstd, wd, dw, db, dcol=dcol, period=period, want_bf16=True, drop_out=s_out)
    assert relerr(dx[sel.to(dev)], gx) < 2e-5 and rowerr(dx[sel.to(dev)], gx) < 2e-5
    assert relerr(dxb[sel.to(dev)], gx * k_out) < 6e-3 and rowerr(dxb[sel.to(dev)], gx * k_out) < 6e-3
    assert relerr(dcol, (gx * k_out).sum(0)) < 5e-5
    assert relerr(dw, gw) < 2e-5 and relerr(db, gb) < 2e-5


# ------------------------------------------------------------------------------------------------ deferred stage-2 reductions

@pytest.mark.parametrize("rows,D", [(40, 768), (1154, 1024), (12608, 768)])
def test_deferred_reductions_match_inline(K, rows, D):
    """The engine's backward sets K.DEFERRED: layernorm_bwd (dw, db, dcol), colsum_bf16 and rowscale_cast_colsum then leave their
    partial rows in private workspaces, and reduce_partials_multi adds all three up in ONE launch later.  Inline, each call reduces
    its own partial rows right away (reduce_partials_kernel).  The stage-1 outputs and partial rows are bit-identical; stage 2 is
    held against the float64 sum of those very partial rows (fp32 summation bound), against float64 of the whole operation, and
    bit for bit against the inline result where both reducers add the same partials in the same order (<= 4 partial rows)."""
    x = rnd(rows, D, seed=21, scale=2.0) + 0.5
    w, b = rnd(D, seed=22) * 0.1 + 1, rnd(D, seed=23) * 0.1
    dy = rnd(rows, D, seed=24)
    yb16 = bf(rnd(rows, D, seed=25))
    g = rnd(rows, D, seed=26)
    rs = (torch.rand(rows, generator=torch.Generator().manual_seed(27)) > 0.2).float() * 1.25
    xd, wd, bd, dyd, ybd, gd, rsd = (t.to(dev) for t in (x, w, b, dy, yb16, g, rs))
    _, _, mean, rstd = K.layernorm_fwd(xd, wd, bd, EPS, want_bf16=False)
    init = (0.5, -0.25, 0.125, 2.0, -1.0)                      # the outputs accumulate (+=) onto what is there

    def run(defer):
        outs = [torch.full((D,), v, device=dev) for v in init]
        parts = []
        K.DEFERRED = [] if defer else None
        try:
            dx, _ = K.layernorm_bwd(dyd, xd, mean, rstd, wd, outs[0], outs[1], dcol=outs[2])
            if not defer:
                parts.append(K.workspace(xd.device, 0)[:(rows + 15) // 16 * 3 * D].clone())
            K.colsum_bf16(ybd, outs[3])
            if not defer:
                parts.append(K.workspace(xd.device, 0)[:(rows + 63) // 64 * D].clone())
            dxb = K.rowscale_cast_colsum(gd, outs[4], rowscale=rsd)
            if not defer:
                parts.append(K.workspace(xd.device, 0)[:(rows + 31) // 32 * D].clone())
            items = K.DEFERRED
        finally:
            K.DEFERRED = None
        if defer:
            assert len(items) == 3 and all(float(o.sub(v).abs().max()) == 0.0 for o, v in zip(outs, init))   # nothing reduced yet
            parts = [it[0][:it[1] * it[2] * it[3]].clone() for it in items]
            K.reduce_partials_multi(items)
        return dx, dxb, outs, parts

    dx_i, dxb_i, outs_i, parts_i = run(False)
    dx_d, dxb_d, outs_d, parts_d = run(True)
    assert torch.equal(dx_d, dx_i) and torch.equal(dxb_d, dxb_i)
    for p_i, p_d in zip(parts_i, parts_d):
        assert torch.equal(p_i, p_d)
    nblks = ((rows + 15) // 16, (rows + 63) // 64, (rows + 31) // 32)
    sets = [(parts_d[0], nblks[0], 3, k) for k in range(3)] + [(parts_d[1], nblks[1], 1, 0), (parts_d[2], nblks[2], 1, 0)]
    for j, (part, nblk, nk, k) in enumerate(sets):
        p = part.view(nblk, nk, D)[:, k].double().cpu()
        exact = init[j] + p.sum(0)
        bound = (nblk + 2) * 2.0 ** -24 * (p.abs().sum(0) + abs(init[j])) + 1e-30
        for o in (outs_i[j], outs_d[j]):
            assert bool(((o.double().cpu() - exact).abs() <= bound).all()), j
        if nblk <= 4:
            assert torch.equal(outs_i[j], outs_d[j]), j
        else:
            assert relerr(outs_d[j], outs_i[j].cpu()) < 1e-6, j
    # the whole operation in float64
    xl, wl, bl = (t.double().requires_grad_(True) for t in (x, w, b))
    (ln64(xl, wl, bl)[0] * dy.double()).sum().backward()
    want = (wl.grad, bl.grad, xl.grad.sum(0), yb16.double().sum(0), (g.double() * rs.double()[:, None]).sum(0))
    for j in range(5):
        assert relerr(outs_d[j] - init[j], want[j]) < (5e-5 if j == 2 else 2e-5), j
    assert relerr(dx_d, xl.grad) < 2e-5 and rowerr(dx_d, xl.grad) < 2e-5
    assert torch.equal(dxb_d.cpu(), bf(g * rs[:, None]))


# ------------------------------------------------------------------------------------------------ hard negatives inside idx groups

@pytest.mark.parametrize("n", [2, 64, 257, 1024])
def test_sample_negatives_with_groups(K, n):
    """sample_negatives(sim, u, group): candidates sharing the row's group (the retrieval fine-tuning `idx`, xvlm.py:254-259) get
    zero weight.  Groups of 1-4 duplicate ids: the pick never shares the row's group and agrees with the float64 inverse-CDF draw
    under the tie rule of test_cross_entropy_and_sampling.  All-distinct ids == the group-less call, bit for bit.  A batch that is
    one group (every candidate of every row masked) returns each row's own index."""
    gen = torch.Generator().manual_seed(n)
    sim = torch.randn(n, n, generator=gen) * 2.0
    u = torch.rand(n, generator=gen)
    sizes = torch.randint(1, 5, (n,), generator=gen)
    ids = torch.repeat_interleave(torch.arange(n), sizes)[:n]
    group = ids[torch.randperm(n, generator=gen)].long()
    if n == 2:
        group = torch.tensor([3, 5])
    simd, ud = sim.to(dev), u.to(dev)
    pick = K.sample_negatives(simd, ud, group.to(dev)).cpu().long()
    same = group[:, None] == group[None, :]
    rows = torch.arange(n)
    assert bool((pick >= 0).all() and (pick < n).all())
    assert not bool(same[rows, pick].any())
    w = torch.softmax(sim.double(), 1) + 1e-5
    w[same] = 0
    cdf = torch.cumsum(w, 1)
    target = u.double() * cdf[:, -1]
    refpick = (cdf > target.unsqueeze(1)).double().argmax(1)
    for r in (pick != refpick).nonzero().flatten().tolist():
        lo, hi = min(int(pick[r]), int(refpick[r])), max(int(pick[r]), int(refpick[r]))
        # only the two candidates around the target may swap (any zero-weight masked columns between them do not count) ...
        assert float(w[r, lo + 1:hi].sum()) == 0.0, (r, int(pick[r]), int(refpick[r]))
        # ... and only where the target sits within fp32 rounding of the CDF step between them
        assert abs(float(cdf[r, lo] - target[r])) <= 1e-5 * float(cdf[r, -1]), (r, float(cdf[r, lo]), float(target[r]))
    assert float((pick != refpick).double().mean()) <= 0.02
    distinct = K.sample_negatives(simd, ud, torch.arange(n, device=dev) * 7 + 3)
    assert torch.equal(distinct, K.sample_negatives(simd, ud))
    one_group = K.sample_negatives(simd, ud, torch.full((n,), 5, dtype=torch.int64, device=dev)).cpu().long()
    assert torch.equal(one_group, rows)


# ------------------------------------------------------------------------------------------------ packed fp32 vectors

def test_copy_f32_multi(K):
    """x2_copy_f32_multi (the stacked bias vectors of a tower, engine.WeightBank.vector): copies and zero segments (source 0), lengths
    around the 256-element block, more descriptors than one launch takes (96); nothing past a segment is written."""
    gen = torch.Generator().manual_seed(5)
    lens = [1, 255, 256, 257, 768, 2304, 3] * 15
    srcs = [None if i % 5 == 2 else torch.randn(n, generator=gen) for i, n in enumerate(lens)]
    srcd = [None if s is None else s.to(dev) for s in srcs]
    offs = [sum(lens[:i]) + 4 * i for i in range(len(lens))]
    dst = torch.full((offs[-1] + lens[-1] + 4,), float("nan"), device=dev)
    K.copy_f32_multi([(0 if s is None else s.data_ptr(), dst.data_ptr() + 4 * o, n) for s, o, n in zip(srcd, offs, lens)])
    got = dst.cpu()
    for s, o, n in zip(srcs, offs, lens):
        assert torch.equal(got[o:o + n], torch.zeros(n) if s is None else s)
        assert bool(torch.isnan(got[o + n:o + n + 4]).all())


# ------------------------------------------------------------------------------------------------ fp32 column sums

@pytest.mark.parametrize("M,N", [(64, 256), (32, 256), (192, 2), (96, 2), (64, 4), (128, 1024), (1, 1), (257, 300), (1000, 513)])
def test_colsum_f32(K, M, N):
    """x2_colsum_f32 (the bias gradient of the fp32 head linears, engine.LinearF32Fn: projections [B, 256], ITM [3B, 2], box
    [B, 4] and hidden MLP layers) plus ragged M and N: out += column sums, against float64 with the fp32 summation bound."""
    x = rnd(M, N, seed=M * 7 + N)
    out = torch.full((N,), 0.25, device=dev)
    K.colsum_f32(x.to(dev), out)
    exact = 0.25 + x.double().sum(0)
    assert relerr(out, exact) < 1e-5
    bound = (M + 2) * 2.0 ** -24 * (x.double().abs().sum(0) + 0.25)
    assert bool(((out.double().cpu() - exact).abs() <= bound).all())
