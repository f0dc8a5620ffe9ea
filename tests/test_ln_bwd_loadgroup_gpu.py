"""x2_layernorm_bwd against float64 at the shapes where its row loop takes another path.

The kernel issues every load of a row before the first arithmetic on it (csrc/rowwise.hip, the rule at the head of the LayerNorm backward section):
D = 256 * NV (256, 768, 1024) runs the form without column guards, a ragged D (260, 1000) the form that clamps the column to the row's last float4, D = 8 has
fewer columns than one lane group.  Rows: fewer than the workgroup's 4 waves (1, 3), one per wave (4), a wave with two rows (5), one full 16-row
block, a ragged second block (17), three blocks (33).  Modes as the training step dispatches them: fp32 dy + dres + bf16 copy, bf16 dy + dres,
fp32 dy + dcol without dres, post (by-products of the final output) with and without a row scale that contains zeros; period 0 / 4 with the skipped
rows untouched; defer 0 / 1, the deferred partial rows added by reduce_partials_multi.  At D = 768 also the input-side and output-side dropout masks,
mirrored on the host as tests/test_kernel_variants_gpu.py does.

Bounds are those of tests/test_kernel_extents_gpu.py, relative to the reference's max-abs (`relerr`): dx 2e-5, dw / db 2e-5, dcol 5e-5, bf16 copy 6e-3."""
import pytest
import torch

from kernel_helpers import BF16, F32, K, bf, relerr, rnd  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
dev = "cuda"
ROWS = [1, 3, 4, 5, 16, 17, 33]
DS = [8, 256, 260, 768, 1000, 1024]
SENT = 777.0            # what dx / the bf16 copy hold before the call: a skipped row must still hold it


def inputs(rows, D, period):
    total = rows if period == 0 else (rows + period - 1) // period * (period + 1)
    sel = torch.arange(rows) if period == 0 else torch.tensor([r + r // period + 1 for r in range(rows)])
    skip = torch.tensor(sorted(set(range(total)) - set(sel.tolist())), dtype=torch.long)
    seed = rows * 4099 + D + period
    x = rnd(total, D, seed=seed, scale=2.0) + 0.5
    w = rnd(D, seed=seed + 1) * 0.1 + 1
    xs = x.double()[sel]
    mean = xs.mean(1).float()
    rstd = (1.0 / torch.sqrt(xs.var(1, unbiased=False) + 1e-6)).float()
    dy, dres = rnd(total, D, seed=seed + 2), rnd(total, D, seed=seed + 3)
    rowscale = (torch.rand(total, generator=torch.Generator().manual_seed(seed + 4)) > 0.3).float() * 1.25
    rowscale[0] = 0.0
    return total, sel, skip, x, w, mean, rstd, dy, dres, rowscale


def reference(x, w, mean, rstd, dyv, sel, mask_in=None):
    """float64 on the kernel's own inputs (the saved fp32 statistics): (dx without dres, dw, db)"""
    d = dyv.double()[sel] * (1.0 if mask_in is None else mask_in)
    xhat = (x.double()[sel] - mean.double()[:, None]) * rstd.double()[:, None]
    g = d * w.double()
    dx = rstd.double()[:, None] * (g - g.mean(1, keepdim=True) - xhat * (g * xhat).mean(1, keepdim=True))
    return dx, (d * xhat).sum(0), d.sum(0)


def run(K, case, dyt, use_dres, want_bf, use_dcol, post, use_rs, defer, period, drop_in=None, drop_out=None):
    """-> (dx, dxb, dw, db, dcol) after one x2_layernorm_bwd through kernels.layernorm_bwd; dw / db / dcol start at 0.5"""
    total, sel, skip, x, w, mean, rstd, dy, dres, rowscale = case
    D = x.shape[1]
    dyv = dy if dyt == "f32" else bf(dy)
    dw, db, dcol = (torch.full((D,), 0.5, device=dev) for _ in range(3))
    dx = torch.full((total, D), SENT, device=dev)
    kw = dict(period=period, dx=dx, want_bf16=want_bf)
    if use_dres:
        kw["dres"] = dres.to(dev)
    if post:
        kw["post"] = (rowscale.to(dev) if use_rs else None, dcol)
    elif use_dcol:
        kw["dcol"] = dcol
    if drop_in is not None:
        kw["drop_in"] = drop_in
    if drop_out is not None:
        kw["drop_out"] = drop_out
    K.DEFERRED = [] if defer else None
    try:
        _, dxb = K.layernorm_bwd(dyv.to(dev), x.to(dev), mean.to(dev), rstd.to(dev), w.to(dev), dw, db, **kw)
        items = K.DEFERRED
    finally:
        K.DEFERRED = None
    if defer:
        torch.cuda.synchronize()
        assert float(dw.min()) == 0.5 and float(dw.max()) == 0.5          # stage 1 alone adds nothing
        assert len(items) == 1
        K.reduce_partials_multi(items)
    torch.cuda.synchronize()
    return dyv, dx, dxb, dw, db, dcol


def untouched(t, rows):
    return rows.numel() == 0 or bool((t[rows.to(t.device)] == torch.tensor(SENT, dtype=t.dtype)).all())      # SENT as the buffer's dtype rounds it


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("period", [0, 4])
@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_bwd_loadgroup(K, rows, D, period, defer):
    case = inputs(rows, D, period)
    total, sel, skip, x, w, mean, rstd, dy, dres, rowscale = case
    # (dy dtype, dres, bf16 copy, dcol, post, post row scale)
    modes = [("f32", True, True, False, 0, False), ("bf16", True, False, False, 0, False), ("f32", False, False, True, 0, False)]
    if period == 0:                 # post = 1 takes period 0 (X2_REQUIRE)
        modes += [("bf16", True, True, True, 1, False), ("bf16", True, True, True, 1, True)]
    selg = sel.to(dev)
    for dyt, use_dres, want_bf, use_dcol, post, use_rs in modes:
        mode = (dyt, use_dres, want_bf, use_dcol, post, use_rs)
        dyv, dx, dxb, dw, db, dcol = run(K, case, dyt, use_dres, want_bf, use_dcol, post, use_rs, defer, period)
        g, dw_ref, db_ref = reference(x, w, mean, rstd, dyv, sel)
        full = g + (dres.double()[sel] if use_dres else 0.0)
        e = {"dx": relerr(dx[selg], full), "dw": relerr(dw - 0.5, dw_ref), "db": relerr(db - 0.5, db_ref)}
        assert e["dx"] < 2e-5 and e["dw"] < 2e-5 and e["db"] < 2e-5, (mode, e)
        assert untouched(dx, skip), mode
        scale = rowscale.double()[sel][:, None] if use_rs else 1.0
        if want_bf:
            want_b = full * scale if post else g
            assert relerr(dxb[selg], want_b) < 6e-3, mode
        else:
            assert dxb is None, mode
        if use_dcol:
            want_c = (full * scale).sum(0) if post else g.sum(0)
            assert relerr(dcol - 0.5, want_c) < 5e-5, (mode, relerr(dcol - 0.5, want_c))
        else:
            assert float(dcol.min()) == 0.5 and float(dcol.max()) == 0.5, mode


@pytest.mark.parametrize("period", [0, 4])
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_bwd_loadgroup_bf16_copy_skips_rows(K, rows, period):
    """the bf16 copy through the C ABI on a pre-filled buffer: the rows a period skips keep what they held (D = 768 and the ragged 1000)"""
    for D in (768, 1000):
        total, sel, skip, x, w, mean, rstd, dy, dres, rowscale = inputs(rows, D, period)
        dxb = torch.full((total, D), SENT, device=dev, dtype=BF16)
        dx = torch.full((total, D), SENT, device=dev)
        dw, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        ws = torch.empty((rows + 15) // 16 * 3 * D, device=dev)
        t = [v.to(dev) for v in (dy, x, mean, rstd, w, dres)]
        K.call("x2_layernorm_bwd", K.ptr(t[0]), 0, K.ptr(t[1]), K.ptr(t[2]), K.ptr(t[3]), K.ptr(t[4]), K.ptr(t[5]), K.ptr(dx), K.ptr(dxb), K.ptr(dw), K.ptr(db),
               None, rows, D, period, 0, 0, 1.0, 0, 0, 1.0, None, K.ptr(ws), 0, 0, None)
        torch.cuda.synchronize()
        g, _, _ = reference(x, w, mean, rstd, dy, sel)
        assert relerr(dxb[sel.to(dev)], g) < 6e-3 and relerr(dx[sel.to(dev)], g + dres.double()[sel]) < 2e-5
        assert untouched(dxb, skip) and untouched(dx, skip)


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("period", [0, 4])
@pytest.mark.parametrize("rows", ROWS)
def test_layernorm_bwd_loadgroup_dropout(K, rows, period, defer):
    """D = 768.  drop_in: the forward dropped the LN output, the incoming gradient carries that mask (dx, dw, db).  drop_out: the bf16 copy and dcol
    carry the mask of the producing linear's dropped output, the fp32 dx does not (no dres with an output mask)."""
    D = 768
    case = inputs(rows, D, period)
    total, sel, skip, x, w, mean, rstd, dy, dres, rowscale = case
    s_in, s_out = K.dropout_spec(0.1, 4321 + rows, 2), K.dropout_spec(0.15, 977 + rows, 9)
    idx = sel.to(torch.int64)[:, None] * D + torch.arange(D, dtype=torch.int64)[None, :]
    k_in, k_out = K.dropout_keep(s_in, idx).double(), K.dropout_keep(s_out, idx).double()
    selg = sel.to(dev)
    dyv, dx, dxb, dw, db, dcol = run(K, case, "f32", True, False, False, 0, False, defer, period, drop_in=s_in)
    g, dw_ref, db_ref = reference(x, w, mean, rstd, dyv, sel, mask_in=k_in)
    assert relerr(dx[selg], g + dres.double()[sel]) < 2e-5 and untouched(dx, skip)
    assert relerr(dw - 0.5, dw_ref) < 2e-5 and relerr(db - 0.5, db_ref) < 2e-5
    dyv, dx, dxb, dw, db, dcol = run(K, case, "f32", False, True, True, 0, False, defer, period, drop_out=s_out)
    g, dw_ref, db_ref = reference(x, w, mean, rstd, dyv, sel)
    assert relerr(dx[selg], g) < 2e-5 and untouched(dx, skip)
    assert relerr(dxb[selg], g * k_out) < 6e-3
    assert relerr(dcol - 0.5, (g * k_out).sum(0)) < 5e-5
    assert relerr(dw - 0.5, dw_ref) < 2e-5 and relerr(db - 0.5, db_ref) < 2e-5
