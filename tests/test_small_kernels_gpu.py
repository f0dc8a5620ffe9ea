"""The head, glue and optimizer kernels (csrc/heads.hip, the token / relative-position kernels of csrc/rowwise.hip, csrc/optim.hip)
against float64 restatements on the CPU, at the shapes where such kernels go wrong: one element, one short of / exactly at / one past
a wavefront, a workgroup, a tile or a chunk, more than one workgroup, ragged tails, misaligned pointers, padded leading dimensions.

Metric: the whole-tensor `relerr` AND `slice_relerr` (row by row / slice by slice, rows at different scales where that is natural),
so that a wrong row cannot hide behind a larger one.  Tolerances are those of tests/test_kernels_gpu.py: 1e-5 of max-abs for fp32
outputs, 1e-6 where the operation is a copy or one add, torch.equal where it is exact, 6e-3 for bf16 outputs; the optimizer keeps
the bounds of tests/test_optim_gpu.py (norm 1e-4 relative, parameters 2e-5 * max(1, max|ref|)).  Buffers a kernel writes part of
carry a sentinel in the rest; columns a kernel must not read carry NaN."""
import ctypes
import importlib
import math

import pytest
import torch

from kernel_helpers import K, bf, relerr, rnd, slice_relerr  # noqa: F401 (fixtures)
from oracle import x2vlm_oracle as O

pytestmark = pytest.mark.gpu
dev = "cuda"
SENT = 7.5            # sentinel: exactly representable, far from every test value's rounding


def check(name, got, ref, tol, floor=1e-3):
    """whole-tensor and per-slice error of `got` against the float64 `ref` (dim 0 = the slices), both held to `tol`"""
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got.float()).all()), name
    whole, sl = relerr(got, ref), slice_relerr(got, ref, floor)
    print("%-40s relerr %.3e  slice_relerr %.3e  (bound %.0e)" % (name, whole, sl, tol))
    assert whole < tol and sl < tol, (name, whole, sl, tol)


def row_scales(n, lo=-2.0, hi=2.0):
    """n factors from 10^lo to 10^hi (1 for a single row)"""
    return torch.logspace(lo, hi, n, dtype=torch.float32) if n > 1 else torch.ones(1)


# ------------------------------------------------------------------------------------------------------------------ l2norm

@pytest.mark.parametrize("D", [1, 32, 63, 64, 65, 256, 1000])
@pytest.mark.parametrize("R", [1, 4, 5, 257])
def test_l2norm_forward_backward(K, R, D):
    """one wave per row, four rows per workgroup: R = 1 / 4 / 5 / 257 is a partial workgroup, a full one, one row into the second and
    65 workgroups; D walks the lane loop `d += 64` through less than one trip, 63 / 64 / 65, four trips (the step's 256) and a ragged
    sixteenth.  Rows scaled from 1e-2 to 1e2 (the output is scale free, the gradient goes with 1 / ||x||)."""
    x = rnd(R, D, seed=100 + D) * row_scales(R)[:, None]
    dy = rnd(R, D, seed=200 + D)
    xl = x.double().requires_grad_(True)
    nrm = xl.norm(dim=1, keepdim=True).clamp_min(1e-12)
    y = xl / nrm
    y.backward(dy.double())
    got_y, got_dx = K.l2norm(x.to(dev)), K.l2norm(x.to(dev), dy.to(dev))
    check("l2norm fwd R=%d D=%d" % (R, D), got_y, y.detach(), 1e-5, floor=0.0)
    if D == 1:
        # y = sign(x): the gradient is dy / |x| - x * (x dy / |x|^2) / |x| = 0, formed from two equal terms of size |dy| / |x| - the
        # float64 reference is 0 (or 1e-17 of that size), so the error is held to 1e-5 of the terms that cancel, row by row
        term = (dy.double() / x.double().abs()).abs()
        err = (got_dx.cpu().double() - xl.grad).abs() / term
        print("l2norm bwd R=%d D=1: error / cancelling term %.3e" % (R, float(err.max())))
        assert float(err.max()) < 1e-5
    else:
        check("l2norm bwd R=%d D=%d" % (R, D), got_dx, xl.grad, 1e-5, floor=0.0)


def test_l2norm_all_zero_row_gives_zeros(K):
    """x / max(||x||, 1e-12) of a zero row is a zero row (forward only: the clamp is there for it), the rows around it unharmed"""
    x = rnd(5, 65, seed=7)
    x[2] = 0.0
    got = K.l2norm(x.to(dev)).cpu()
    assert float(got[2].abs().max()) == 0.0
    keep = [0, 1, 3, 4]
    check("l2norm fwd around a zero row", got[keep], x[keep].double() / x[keep].double().norm(dim=1, keepdim=True), 1e-5, floor=0.0)


# ------------------------------------------------------------------------------------------------------------------ cross-entropy

def ce_case(R, C, ld, seed, all_ignored=False):
    """logits randn * 3 with row 1 (row 0 when R == 1) moved by +80 and row 2 by -80 (a missing max subtraction overflows / underflows
    there), NaN in the pad columns C..ld-1 (must not be read), labels random; the first and the last row ignored (-100) when there are
    at least five rows.  The labels of the two moved rows sit on their smallest logit: (softmax - onehot) then has an entry of
    size ~1 and the row is held to its full scale (a row whose label carries nearly all the probability has a gradient of
    (p - 1) ~ 0 by cancellation)."""
    z = torch.full((R, ld), float("nan"))
    z[:, :C] = rnd(R, C, seed=seed, scale=3.0)
    lab = torch.randint(0, C, (R,), generator=torch.Generator().manual_seed(seed + 1))
    moved = [0] if R == 1 else ([1, 2] if R >= 3 else [])
    for r, off in zip(moved, (80.0, -80.0)):
        z[r, :C] += off
        lab[r] = int(z[r, :C].argmin())
    if R >= 5:
        lab[0] = -100
        lab[-1] = -100
    if all_ignored:
        lab[:] = -100
    return z, lab


CE_SHAPES = [(1, 2, 2), (300, 2, 2), (20, 3, 64), (7, 255, 256), (7, 256, 256), (7, 257, 320), (600, 1000, 1024), (5, 4096, 4096)]


@pytest.mark.parametrize("R,C,ld", CE_SHAPES, ids=["R%d_C%d_ld%d" % s for s in CE_SHAPES])
def test_cross_entropy_forward_backward(K, R, C, ld):
    """x2_ce_fwd / x2_ce_bwd: C = 2 (the ITM head) and 3 sit below one wavefront, 255 / 256 / 257 around the workgroup's column loop,
    4096 takes sixteen trips; R = 300 and 600 take the second and third trip of ce_reduce_kernel's `r += 256` loop; ld > C pads."""
    z, lab = ce_case(R, C, ld, seed=300 + R + C)
    zz = z[:, :C].double()
    valid = lab >= 0
    ref_lse = torch.logsumexp(zz, -1)
    ref_rows = (ref_lse - zz[torch.arange(R), lab.clamp_min(0)])[valid]
    ref_loss, count = float(ref_rows.sum() / ref_rows.numel()), int(valid.sum())
    zd, ld_ = z.to(dev), lab.to(dev)
    stat, lse = K.ce_fwd(zd, ld_, C_valid=C)
    stat2, lse2 = K.ce_fwd(zd, ld_, C_valid=C)
    assert torch.equal(stat, stat2) and torch.equal(lse, lse2)             # fixed-order sums: the same bits on every run
    check("ce lse", lse.view(R, 1), ref_lse.view(R, 1), 1e-5)
    print("ce stat[0] %.8f ref %.8f" % (float(stat[0]), ref_loss))
    assert abs(float(stat[0]) - ref_loss) < 1e-5 * abs(ref_loss)
    assert float(stat[1]) == float(count)
    g, gscale = torch.tensor([0.7], device=dev), 0.5
    ref_dl = torch.softmax(zz, -1)
    ref_dl[torch.arange(R), lab.clamp_min(0)] -= 1.0
    ref_dl = ref_dl * (gscale * float(torch.tensor(0.7)) / count) * valid.double().unsqueeze(1)
    for dtype, tol in ((torch.float32, 1e-5), (torch.bfloat16, 6e-3)):
        dl = K.ce_bwd(zd, ld_, lse, g, stat, C_valid=C, gscale=gscale, out_dtype=dtype)
        assert dl.dtype == dtype and dl.shape == (R, ld)
        # floor 0.05 (as the attention tests use): every entry is a difference of two numbers in [0, 1] times the common scale, so a
        # row that cancels to (near) nothing is held to 5 % of the tensor's max-abs, not to its own
        check("ce dl %s" % str(dtype)[6:], dl[:, :C], ref_dl, tol, floor=0.05)
        if dtype == torch.float32:                    # for the record: the same expression evaluated by torch in fp32 on the CPU
            t32 = torch.softmax(z[:, :C], -1)
            t32[torch.arange(R), lab.clamp_min(0)] -= 1.0
            t32 = t32 * (gscale * torch.tensor(0.7) / count) * valid.float().unsqueeze(1)
            print("   (fp32 torch evaluation: relerr %.3e  slice_relerr %.3e)" % (relerr(t32, ref_dl), slice_relerr(t32, ref_dl, 0.05)))
        if ld > C:
            assert float(dl[:, C:].float().abs().max()) == 0.0                # pad columns: exactly zero, and the NaNs there were not read
        if count < R:
            assert float(dl[~valid.to(dev)].float().abs().max()) == 0.0       # ignored rows: exactly zero


def test_cross_entropy_with_every_label_ignored(K):
    """no counted row: the mean over nothing is 0 / 0 = NaN, exactly what torch.nn.functional.cross_entropy returns for such a batch
    (asserted here, so the reason for the expectation is on record); the count is 0 and the gradient is all zeros, not NaN"""
    R, C, ld = 7, 255, 256
    z, lab = ce_case(R, C, ld, seed=77, all_ignored=True)
    assert math.isnan(float(torch.nn.functional.cross_entropy(z[:, :C], lab, ignore_index=-100)))
    stat, lse = K.ce_fwd(z.to(dev), lab.to(dev), C_valid=C)
    assert math.isnan(float(stat[0])) and float(stat[1]) == 0.0
    check("ce lse (all ignored)", lse.view(R, 1), torch.logsumexp(z[:, :C].double(), -1).view(R, 1), 1e-5)
    g = torch.tensor([0.7], device=dev)
    for dtype in (torch.float32, torch.bfloat16):
        dl = K.ce_bwd(z.to(dev), lab.to(dev), lse, g, stat, C_valid=C, gscale=0.5, out_dtype=dtype)
        assert float(dl.float().abs().max()) == 0.0                           # abs().max() of a NaN is NaN: this also rules NaN out


# ------------------------------------------------------------------------------------------------------------------ linear_f32

# every M, N of {1, 63, 64, 65, 130} and every K of {1, 15, 16, 17, 127, 128, 129, 1000}; the wrapper cuts the contraction into
# slices when K >= 128 and the output has fewer than 64 tiles (all of these), and runs one pass when K < 128 - or at 64 tiles and more,
# which the last case reaches (8 x 8 tiles) with a K that would otherwise be split
LINEAR_SHAPES = [(1, 1, 1), (63, 65, 15), (64, 64, 16), (65, 63, 17), (130, 1, 127), (1, 130, 128), (63, 64, 129), (64, 130, 1000),
                 (130, 63, 1000), (65, 65, 128), (450, 460, 129)]


@pytest.mark.parametrize("transA,transB", [(False, False), (True, False), (False, True), (True, True)], ids=["nn", "tn", "nt", "tt"])
@pytest.mark.parametrize("M,N,Kd", LINEAR_SHAPES, ids=["M%d_N%d_K%d" % s for s in LINEAR_SHAPES])
def test_linear_f32(K, M, N, Kd, transA, transB):
    """x2_linear_f32: ragged tiles in M and N, a last K step that is partial (K % 16 != 0: the `k < kend` guard), A as a column slice
    of a wider tensor, the output as a column slice of a sentinel-filled wider buffer, bias, then accumulate=True onto that result
    with alpha together with a device alpha_ptr (their product applies).  Rows of op(A) scaled from 1e-2 to 1e2."""
    # N = 1: a row is one dot product with nothing beside it to be measured against, and a dot product that cancels is not wrong:
    # there the rows stay at one scale and the metric's slice is the column
    a = rnd(M, Kd, seed=400 + M + Kd) * (row_scales(M)[:, None] if N > 1 else 1.0)   # op(A) [M, K]
    sl = (lambda t: t) if N > 1 else (lambda t: t.t())
    b = rnd(N, Kd, seed=500 + N + Kd, scale=Kd ** -0.5)                      # op(B) [N, K]
    bias = rnd(N, seed=600 + N)
    Aw = torch.full((Kd, M + 5) if transA else (M, Kd + 5), SENT)
    Aw[:, 3:3 + (M if transA else Kd)] = a.t() if transA else a
    Awd = Aw.to(dev)
    A = Awd[:, 3:3 + (M if transA else Kd)]
    B = (b.t().contiguous() if transB else b).to(dev)
    prod = a.double() @ b.double().t()
    tiles = ((M + 63) // 64) * ((N + 63) // 64)
    split = not (tiles >= 64 or Kd < 128)
    outs = []
    for _ in range(2):
        wide = torch.full((M, N + 7), SENT, device=dev)
        K.linear_f32(A, B, bias=bias.to(dev), transA=transA, transB=transB, out=wide[:, 4:4 + N])
        outs.append(wide)
    wide = outs[0]
    assert torch.equal(outs[0], outs[1])                                     # slices added in slice order: the same bits twice
    check("linear %s" % ("split" if split else "one pass"), sl(wide[:, 4:4 + N]), sl(prod + bias.double()), 1e-5)
    assert bool((wide[:, :4] == SENT).all()) and bool((wide[:, 4 + N:] == SENT).all())
    alpha_ptr = torch.tensor([-1.5], device=dev)
    K.linear_f32(A, B, transA=transA, transB=transB, alpha=0.5, alpha_ptr=alpha_ptr, out=wide[:, 4:4 + N], accumulate=True)
    check("linear accumulate, alpha * alpha_ptr", sl(wide[:, 4:4 + N]), sl(prod + bias.double() + (0.5 * -1.5) * prod), 1e-5)
    assert bool((wide[:, :4] == SENT).all()) and bool((wide[:, 4 + N:] == SENT).all())
    assert bool((Awd[:, :3] == SENT).all()) and bool((Awd[:, 3 + (M if transA else Kd):] == SENT).all())


def test_linear_f32_with_empty_contraction_slices(K):
    """through the entry point itself: ksplit = 64 at K = 100 gives slices of 16, so slices 7 .. 63 start past the end (kbeg >= K);
    they must contribute exact zeros - the workspace starts as NaN - and slice 6 is the partial one (k = 96 .. 99)"""
    M, N, Kd, ksplit = 65, 63, 100, 64
    a, b, bias = rnd(M, Kd, seed=1) * row_scales(M)[:, None], rnd(N, Kd, seed=2, scale=0.1), rnd(N, seed=3)
    ad, bd, biasd = a.to(dev), b.to(dev), bias.to(dev)
    outs = []
    for _ in range(2):
        ws = torch.full((ksplit * M * N,), float("nan"), device=dev)
        wide = torch.full((M, N + 7), SENT, device=dev)
        out = wide[:, 4:4 + N]
        K.call("x2_linear_f32", K.ptr(ad), K.ptr(bd), K.ptr(out), K.ptr(biasd), None, 2.0, M, N, Kd, ad.stride(0), ad.stride(1),
               bd.stride(0), bd.stride(1), out.stride(0), 0, ksplit, K.ptr(ws))
        outs.append(wide)
    assert torch.equal(outs[0], outs[1])
    check("linear ksplit=64 K=100", outs[0][:, 4:4 + N], 2.0 * (a.double() @ b.double().t()) + bias.double(), 1e-5)
    assert bool((outs[0][:, :4] == SENT).all()) and bool((outs[0][:, 4 + N:] == SENT).all())


# ------------------------------------------------------------------------------------------------------------------ gelu

@pytest.mark.parametrize("n", [1, 255, 256, 257, 2 ** 20 + 3])
def test_gelu_f32_forward_backward(K, n):
    """x2_gelu_f32: one element, one short of / exactly / one past a workgroup, 4097 workgroups with three elements in the last.  Values:
    1, 0, +-1e-4, +-12, a linspace over [-12, 12] that contains 0, and randn, in a seeded shuffle so that every 256-element chunk (the
    slices of the metric: one workgroup each) spans the range.  Reference: the erf form in float64 and its autograd."""
    special = torch.tensor([1.0, 0.0, 1e-4, -1e-4, -12.0, 12.0])
    nl = max(0, (n - 6) // 2) | 1 if n > 6 else 0
    x = torch.cat([special, torch.linspace(-12.0, 12.0, nl) if nl else torch.zeros(0), rnd(max(0, n - 6 - nl), seed=n)])
    if n >= 6:
        assert x.numel() == n
        x = x[torch.randperm(n, generator=torch.Generator().manual_seed(n))]
    x = x[:n].contiguous()
    dy = rnd(n, seed=n + 1)
    xl = x.double().requires_grad_(True)
    y = 0.5 * xl * (1.0 + torch.erf(xl / math.sqrt(2.0)))
    y.backward(dy.double())
    rows = (n + 255) // 256

    def chunks(t):                                      # [rows, 256], the tail chunk padded with zeros (they add no error)
        out = torch.zeros(rows * 256, dtype=t.dtype)
        out[:n] = t.detach().cpu()
        return out.view(rows, 256)

    check("gelu fwd n=%d" % n, chunks(K.gelu_f32(x.to(dev))), chunks(y), 1e-5)
    check("gelu bwd n=%d" % n, chunks(K.gelu_f32(x.to(dev), dy.to(dev))), chunks(xl.grad), 1e-5)


# ------------------------------------------------------------------------------------------------------------------ gather / scatter rows

@pytest.mark.parametrize("ln", [4, 1028])
def test_gather_and_scatter_rows(K, ln):
    """x2_gather_rows / x2_scatter_rows with rows of one float4 and of 257 (a second column chunk that holds one float4): a single row,
    every index the same, and one destination row fed by 300 sources while others get one or none.  The scatter adds 300 rows at scales
    1e-2 .. 1e2 in ascending order; reference: index_add_ in float64."""
    S = 6
    src = rnd(S, ln, seed=ln) * row_scales(S)[:, None]
    for name, idx in (("R=1", [3]), ("all the same", [2] * 5), ("300 onto one", [1] * 150 + [4, 0] + [1] * 150 + [5])):
        idx_t = torch.tensor(idx, dtype=torch.int32)
        R = len(idx)
        d32, d16 = K.gather_rows(src.to(dev), idx_t.to(dev), ln, want_bf16=True)
        assert d32.shape == (R, ln) and torch.equal(d32.cpu(), src[idx_t.long()]), name
        assert torch.equal(d16.cpu(), bf(src[idx_t.long()])), name
        only16 = K.gather_rows(src.to(dev), idx_t.to(dev), ln, want_f32=False, want_bf16=True)
        assert only16[0] is None and torch.equal(only16[1], d16), name
        up = rnd(R, ln, seed=ln + R) * row_scales(R)[:, None]
        got = K.scatter_rows(up.to(dev), idx_t.to(dev), S, ln)
        ref = torch.zeros(S, ln, dtype=torch.float64).index_add_(0, idx_t.long(), up.double())
        check("scatter_rows len=%d %s" % (ln, name), got, ref, 1e-5)
        untouched = [d for d in range(S) if d not in idx]
        assert float(got[untouched].abs().max()) == 0.0, name                  # every row written: zeros where nothing points
        assert torch.equal(got, K.scatter_rows(up.to(dev), idx_t.to(dev), S, ln)), name


# ------------------------------------------------------------------------------------------------------------------ token kernels

@pytest.mark.parametrize("B,res", [(2, 224), (1, 384)])
def test_patchify_at_the_real_resolutions(K, B, res):
    img = rnd(B, 3, res, res, seed=res)
    g, p = res // 16, 16
    ref = img.view(B, 3, g, p, g, p).permute(0, 2, 4, 1, 3, 5).reshape(B * g * g, 3 * p * p)
    cols = K.patchify(img.to(dev), 16)
    assert cols.shape == ref.shape and torch.equal(cols.cpu(), bf(ref))


@pytest.mark.parametrize("B,P,D", [(1, 196, 768), (3, 576, 1024)])
def test_assemble_tokens_forward_backward(K, B, P, D):
    """copies are exact; dcls += the B class-token rows, in ascending b (one add at B = 1)"""
    patch, cls = rnd(B * P, D, seed=P) * row_scales(B * P)[:, None], rnd(D, seed=P + 1)
    x = K.assemble_tokens(patch.to(dev), cls.to(dev), B, P)
    assert torch.equal(x.cpu(), torch.cat([cls.expand(B, 1, D), patch.view(B, P, D)], 1))
    dx = rnd(B, P + 1, D, seed=P + 2) * row_scales(B)[:, None, None]
    init = rnd(D, seed=P + 3)
    outs = []
    for _ in range(2):
        dcls = init.clone().to(dev)
        dpatch = K.assemble_tokens_bwd(dx.to(dev), dcls)
        outs.append((dpatch, dcls))
    assert torch.equal(outs[0][0].cpu(), bf(dx[:, 1:].reshape(B * P, D)))
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[1][0])
    check("assemble_tokens_bwd dcls", outs[0][1].view(1, D), (init.double() + dx[:, 0].double().sum(0)).view(1, D), 1e-6 if B == 1 else 1e-5)


@pytest.mark.parametrize("D", [768, 1000])
def test_pool_tokens_at_196_patches(K, D):
    """x2_pool_tokens at P = 196 (four waves x 49 patches), D = 768 and a D whose last 256-column workgroup is ragged: uniform weights,
    0 / 1 weights, and a sample whose only kept patch is the first.  Forward: a 196-term weighted mean (1e-5); backward: one
    multiply-add per element (1e-6) and a zeroed token-0 row."""
    B, P = 3, 196
    x = rnd(B, P + 1, D, seed=D) * row_scales(B)[:, None, None]
    w01 = (torch.rand(B, P, generator=torch.Generator().manual_seed(D)) > 0.5).float()
    w01[1] = 0.0
    w01[1, 0] = 1.0
    w01[2, -1] = 1.0
    for name, w in (("uniform", None), ("0/1", w01)):
        ww = (torch.ones(B, P) if w is None else w).double()
        wd = None if w is None else w.to(dev)
        got = K.pool_tokens(x.clone().to(dev), wd)
        pooled = (ww.unsqueeze(-1) * x[:, 1:].double()).sum(1) / ww.sum(1, keepdim=True)
        check("pool_tokens fwd %s" % name, got[:, 0], pooled, 1e-5)
        assert torch.equal(got[:, 1:].cpu(), x[:, 1:])                                    # the patch rows are read only
        if w is not None:
            check("pool_tokens fwd: the sample that keeps one patch", got[1:2, 0], x[1:2, 1].double(), 1e-6)
        gg = K.pool_tokens(x.clone().to(dev), wd, bwd=True)
        refg = x[:, 1:].double() + (ww / ww.sum(1, keepdim=True)).unsqueeze(-1) * x[:, :1].double()
        check("pool_tokens bwd %s" % name, gg[:, 1:], refg, 1e-6)
        assert float(gg[:, 0].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------------ relative-position bias

@pytest.mark.parametrize("H", [12, 16])
@pytest.mark.parametrize("window", [14, 24])
def test_relpos_bias_forward(K, window, H):
    """x2_relpos_bias at the 224-px and 384-px windows (N = 197 -> ld 256, N = 577 -> ld 640): bias[h][i][j] = table[index[i][j]][h]
    and its transpose are copies (exact), the pad columns N .. ld-1 of both are zeros (the buffers start as NaN), the log2-unit
    tables are the plain ones times log2(e), and the three ways in (wrapper; entry point with the transposed index; entry point
    scattering the transpose, with and without a transposed output) write the same tables."""
    idx = O.relative_position_index(window)
    N, T = idx.shape[0], int(idx.max()) + 1
    ld = K.round_up(N, 64)
    table = rnd(T, H, seed=window + H) * row_scales(T, -1.0, 1.0)[:, None]
    ref = table[idx.reshape(-1)].view(N, N, H).permute(2, 0, 1).contiguous()
    td, idd = table.to(dev), idx.to(dev)
    idT = idd.t().contiguous()

    def direct(indexT, want_T, scale):
        bias = torch.full((H, N, ld), float("nan"), device=dev)
        biasT = torch.full((H, N, ld), float("nan"), device=dev) if want_T else None
        K.call("x2_relpos_bias", K.ptr(td), K.ptr(idd), K.ptr(indexT), K.ptr(bias), K.ptr(biasT), N, H, ld, ld, scale)
        return bias, biasT

    plain = {}
    for log2 in (False, True):
        bias, biasT = direct(idT, True, K.LOG2E if log2 else 1.0)
        assert float(bias[:, :, N:].abs().max()) == 0.0 and float(biasT[:, :, N:].abs().max()) == 0.0      # NaN would fail this too
        if not log2:
            assert torch.equal(bias[:, :, :N].cpu(), ref) and torch.equal(biasT[:, :, :N].cpu(), ref.transpose(1, 2))
            plain = (bias, biasT)
        else:
            check("relpos bias log2", bias[:, :, :N], ref.double() * K.LOG2E, 1e-6)
            check("relpos biasT log2", biasT[:, :, :N], ref.transpose(1, 2).double() * K.LOG2E, 1e-6)
            check("relpos bias log2 vs plain", bias, plain[0].cpu().double() * K.LOG2E, 1e-6)
            check("relpos biasT log2 vs plain", biasT, plain[1].cpu().double() * K.LOG2E, 1e-6)
        wb, wT = K.relpos_bias(td, idd, log2=log2)
        assert torch.equal(wb, bias) and torch.equal(wT, biasT)
        sb, sT = direct(None, True, K.LOG2E if log2 else 1.0)
        assert torch.equal(sb, bias) and torch.equal(sT, biasT)
        ob, oT = direct(None, False, K.LOG2E if log2 else 1.0)
        assert oT is None and torch.equal(ob, bias)


# ------------------------------------------------------------------------------------------------------------------ frame mean

@pytest.mark.parametrize("Bc,F,T,D", [(2, 8, 197, 768), (1, 1, 5, 64), (3, 4, 33, 1024)])
def test_frame_mean_forward_backward(K, Bc, F, T, D):
    """x2_frame_mean: the 8-frame clip at the real token geometry, the smallest problem (one frame: a copy plus one add, 80 float4 in one
    workgroup) and an odd token count at D = 1024; forward, dx and dpos (a Bc * T-row column sum in four fixed slices) against float64
    autograd of mean_f(x + pos)."""
    x = rnd(Bc * F, T, D, seed=F) * row_scales(Bc * F)[:, None, None]
    pos, dy = rnd(F, D, seed=F + 1), rnd(Bc, T, D, seed=F + 2) * row_scales(Bc)[:, None, None]
    xl, pl = x.double().requires_grad_(True), pos.double().requires_grad_(True)
    ref = (xl.view(Bc, F, T, D) + pl.view(1, F, 1, D)).mean(1)
    ref.backward(dy.double())
    out = K.frame_mean(x.to(dev), pos.to(dev), F)
    check("frame_mean fwd", out, ref.detach(), 1e-6 if F == 1 else 1e-5)
    check("frame_mean fwd, no position rows", K.frame_mean(x.to(dev), None, F), x.double().view(Bc, F, T, D).mean(1), 1e-6 if F == 1 else 1e-5)
    dx, dpos = K.frame_mean_bwd(dy.to(dev), F)
    dx2, dpos2 = K.frame_mean_bwd(dy.to(dev), F)
    assert torch.equal(dx, dx2) and torch.equal(dpos, dpos2)
    check("frame_mean dx", dx, xl.grad, 1e-6)
    check("frame_mean dpos", dpos, pl.grad, 1e-5)
    assert K.frame_mean_bwd(dy.to(dev), F, want_dpos=False)[1] is None


# ------------------------------------------------------------------------------------------------------------------ embeddings / tables

@pytest.mark.parametrize("D", [768, 1024])
def test_embed_fwd(K, D):
    """x2_embed_fwd: 7 sequences of 30 tokens, one workgroup per token row, 192 / 256 float4 per row; ids include 0 and V - 1"""
    V, L, Bn = 50, 30, 7
    ids = torch.randint(0, V, (Bn, L), generator=torch.Generator().manual_seed(D))
    ids[0, 0], ids[-1, -1], ids[3, 7] = 0, V - 1, V - 1
    word, pos, typ = rnd(V, D, seed=1) * row_scales(V)[:, None], rnd(40, D, seed=2), rnd(2, D, seed=3)
    out = K.embed_fwd(ids.to(dev), word.to(dev), pos.to(dev), typ.to(dev))
    ref = word.double()[ids.reshape(-1)] + pos.double()[:L].repeat(Bn, 1) + typ.double()[0]
    check("embed_fwd D=%d" % D, out, ref, 1e-6)


@pytest.mark.parametrize("B,L,T", [(1, 30, 197), (64, 30, 197)])
def test_tail_index(K, B, L, T):
    """x2_tail_index at the step's text / image lengths, one sample and the step's 64 (256 workgroups): exact against the cat / index
    expressions it replaces, with and without the match rows"""
    g = torch.Generator().manual_seed(B)
    ineg = torch.randint(0, B, (B,), generator=g, dtype=torch.int32)
    tneg = torch.randint(0, B, (B,), generator=g, dtype=torch.int32)
    ta = (torch.rand(B, L, generator=g) > 0.3).long()
    ia = (torch.rand(B, T, generator=g) > 0.2).long()
    ar = torch.arange(B, dtype=torch.int32)
    for with_match in (True, False):
        t_idx, kv, atts, enc = K.tail_index(ineg.to(dev) if with_match else None, tneg.to(dev) if with_match else None, ta.to(dev), ia.to(dev),
                                            with_match=with_match)
        ti = torch.cat([ar, ar, tneg, ar + B]) if with_match else ar + B
        ki = torch.cat([ar, ineg, ar, ar]) if with_match else ar
        assert torch.equal(t_idx.cpu(), ti) and torch.equal(kv.cpu(), ki)
        assert torch.equal(atts.cpu(), torch.cat([ta, ta])[ti.long()]) and torch.equal(enc.cpu(), ia[ki.long()])


# ------------------------------------------------------------------------------------------------------------------ optimizer

CHUNK = 16384          # elements per workgroup of gradsq_kernel / adamw_kernel (OPT_CHUNK, csrc/optim.hip)


def hf_adamw_step(p, g, m, v, t, lr, wd, b1=0.9, b2=0.98, eps=1e-8):
    """transformers 4.12.5 AdamW.step for one tensor (float64 maths on CPU)."""
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    denom = v.sqrt().add_(eps)
    step = lr * math.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    p.addcdiv_(m, denom, value=-step)
    p.add_(p, alpha=-lr * wd)


def run_optimizer(params, group_of, hyper, grads_of_step, clip, piece=None):
    """`steps` iterations of optim.FusedAdamW on `params` (device) beside the float64 HuggingFace rule on the CPU.
    group_of[i]: parameter group of tensor i, hyper[g] = (lr, weight_decay); grads_of_step(t) -> list of device gradients (None:
    no gradient this step, the tensor's own step count stays behind); clip: None = step() alone (the kernel gets no clip pointer),
    otherwise max_norm of grad_norm() before every step (0: no clipping, the coefficient is 1).  After every step the norm is held to
    1e-4 relative and every parameter to 2e-5 * max(1, max|ref|) - per `piece` elements (a 16384-element chunk) where given."""
    optim = importlib.import_module("x2-vlm_amd.optim")
    groups = [{"params": [p for p, gi in zip(params, group_of) if gi == g_], "lr": lr, "weight_decay": wd} for g_, (lr, wd) in enumerate(hyper)]
    opt = optim.FusedAdamW(groups)
    ref = [p.detach().cpu().double().clone() for p in params]
    ms, vs, steps = [torch.zeros_like(r) for r in ref], [torch.zeros_like(r) for r in ref], [0] * len(params)
    worst, t = 0.0, 0
    while True:
        t += 1
        grads = grads_of_step(t)
        if grads is None:
            return worst
        for p, g in zip(params, grads):
            p.grad = g
        tot = math.sqrt(sum(float((g.cpu().double() ** 2).sum()) for g in grads if g is not None))
        coef = 1.0
        if clip is not None:
            norm = opt.grad_norm(max_norm=clip)
            again = opt.grad_norm(max_norm=clip)
            assert torch.equal(norm, again)                                   # block partials added in a fixed order
            assert abs(float(norm[0]) - tot) < 1e-4 * tot, (float(norm[0]), tot)
            coef = min(1.0, clip / (tot + 1e-6)) if clip > 0 else 1.0
            assert abs(float(norm[1]) - coef) < 1e-4 * coef, (float(norm[1]), coef)
        opt.step()
        for i, g in enumerate(grads):
            if g is None:
                continue
            steps[i] += 1
            hf_adamw_step(ref[i], g.cpu().double() * coef, ms[i], vs[i], steps[i], *hyper[group_of[i]])
        for i, (p, r) in enumerate(zip(params, ref)):
            got, n = p.detach().cpu().double().reshape(-1), r.numel()
            for o in range(0, n, piece or n):
                rr = r.reshape(-1)[o:o + (piece or n)]
                err = float((got[o:o + (piece or n)] - rr).abs().max()) / max(1.0, float(rr.abs().max()))
                worst = max(worst, err)
                assert err < 2e-5, (t, i, o, err)


def test_optimizer_misaligned_views(K):
    """Parameters and gradients that are views at element offsets 1, 2 and 3 of one flat buffer each (4, 8, 12 bytes past a 16-byte
    boundary, as views into an arena can be): gradsq_kernel and adamw_kernel take their scalar branch (n4 = 0).  Sizes 1, 3, 5, 16383
    and 16387 (a second chunk of three elements); a sentinel element before and after every view must survive grad_norm() and step()."""
    sizes, offs = [1, 3, 5, 16383, 16387], [1, 2, 3, 1, 2]
    starts, cur = [], 0
    for n, o in zip(sizes, offs):
        cur = (cur + 4) // 4 * 4 + o                    # >= one sentinel element after the previous view, then offset o of a float4
        starts.append(cur)
        cur += n
    total = cur + 4
    pflat, gflat = torch.full((total,), SENT, device=dev), torch.full((total,), SENT, device=dev)
    assert pflat.data_ptr() % 16 == 0 and gflat.data_ptr() % 16 == 0
    inside = torch.zeros(total, dtype=torch.bool)
    params = []
    for i, (s, n) in enumerate(zip(starts, sizes)):
        pflat[s:s + n] = rnd(n, seed=700 + i).to(dev)
        inside[s:s + n] = True
        params.append(torch.nn.Parameter(pflat[s:s + n]))
        assert params[-1].data_ptr() == pflat.data_ptr() + 4 * s and params[-1].data_ptr() % 16 == 4 * offs[i]
    assert not bool(inside[[s - 1 for s in starts]].any()) and not bool(inside[[s + n for s, n in zip(starts, sizes)]].any())

    def grads(t):
        if t > 3:
            return None
        out = []
        for i, (s, n) in enumerate(zip(starts, sizes)):
            gflat[s:s + n] = (rnd(n, seed=800 + 10 * t + i) * (3.0 if t % 2 else 0.1)).to(dev)
            out.append(gflat[s:s + n])
        return out

    worst = run_optimizer(params, [0, 1, 0, 1, 0], [(1e-2, 0.01), (2e-2, 0.0)], grads, clip=1.0, piece=CHUNK)
    print("misaligned views: worst parameter error / max(1, |ref|) %.3e" % worst)
    outside = ~inside.to(dev)
    assert bool((pflat[outside] == SENT).all()) and bool((gflat[outside] == SENT).all())


def test_optimizer_chunk_edges(K):
    """Aligned tensors whose sizes sit on, one short of and one past the 16384-element chunk of a workgroup, two chunks, two chunks and
    one, three chunks and seven; every chunk at its own scale (0.1, 1, 10, 100) and checked on its own, so that a wrong chunk offset
    cannot hide behind a neighbour."""
    sizes = [16383, 16384, 16385, 32768, 32769, 3 * 16384 + 7]

    def scaled(n, seed, base):
        t = rnd(n, seed=seed) * base
        for c in range((n + CHUNK - 1) // CHUNK):
            t[c * CHUNK:(c + 1) * CHUNK] *= 10.0 ** (c - 1)
        return t

    params = [torch.nn.Parameter(scaled(n, 900 + i, 1.0).to(dev)) for i, n in enumerate(sizes)]
    grads = lambda t: None if t > 3 else [scaled(n, 950 + 10 * t + i, 3.0 if t % 2 else 0.1).to(dev) for i, n in enumerate(sizes)]
    worst = run_optimizer(params, [0, 0, 1, 1, 2, 2], [(1e-2, 0.01), (2e-2, 0.0), (5e-3, 0.1)], grads, clip=1.0, piece=CHUNK)
    print("chunk edges: worst chunk error / max(1, |ref|) %.3e" % worst)


@pytest.mark.parametrize("clip", [None, 0.0, 1e6, 1.0], ids=["no_clip_pointer", "max_norm_0", "norm_below_max_norm", "clipped"])
def test_optimizer_many_tensors(K, clip):
    """600 tensors of 1 .. 300 elements (seeded) in 16 parameter groups with their own lr and weight decay - the table's binary search
    runs over as many rows as the model has, every group slot of the kernel's hyper-parameter block is read -, three steps, every
    third tensor without a gradient on step 2 so that the per-tensor step counts diverge.  Unclipped three ways (step() alone,
    max_norm = 0, a norm below max_norm: the coefficient is 1) and clipped."""
    gen = torch.Generator().manual_seed(600)
    sizes = torch.randint(1, 301, (600,), generator=gen).tolist()
    group_of = [i % 16 for i in range(600)]
    hyper = [(1e-3 * (1 + g_), 0.01 * (g_ % 4)) for g_ in range(16)]
    flat = rnd(sum(sizes), seed=601)
    params = [torch.nn.Parameter(t.clone().to(dev)) for t in flat.split(sizes)]
    assert all(p.data_ptr() % 16 == 0 for p in params)

    def grads(t):
        if t > 3:
            return None
        gs = list((rnd(sum(sizes), seed=610 + t) * (3.0 if t % 2 else 0.1)).split(sizes))
        return [None if (t == 2 and i % 3 == 0) else g.clone().to(dev) for i, g in enumerate(gs)]

    worst = run_optimizer(params, group_of, hyper, grads, clip=clip)
    print("600 tensors, clip=%s: worst tensor error / max(1, |ref|) %.3e" % (clip, worst))


def test_argument_checks_return_before_any_launch(K):
    """rejections that the entry points already make on the host (X2_REQUIRE, before the launch): a seventeenth parameter group -
    the kernel's hyper-parameter block has sixteen slots -, more candidates than sample_negatives' 1024-entry LDS row, a row length
    that is not a whole number of float4"""
    lib = importlib.import_module("x2-vlm_amd._lib")
    optim = importlib.import_module("x2-vlm_amd.optim")
    ps = [torch.nn.Parameter(torch.zeros(4, device=dev)) for _ in range(17)]
    with pytest.raises(AssertionError):
        optim.FusedAdamW([{"params": [p], "lr": 1e-3, "weight_decay": 0.0} for p in ps])
    table = torch.zeros(64, dtype=torch.uint8, device=dev)
    lr, wd = (ctypes.c_float * 17)(*([1e-3] * 17)), (ctypes.c_float * 17)(*([0.0] * 17))
    with pytest.raises(lib.X2HipError):
        K.call("x2_adamw_multi", K.ptr(table), 1, 1, lr, wd, 17, 0.9, 0.98, 1e-8, None)
    optim.FusedAdamW([{"params": [p], "lr": 1e-3, "weight_decay": 0.0} for p in ps[:16]])           # sixteen are fine
    with pytest.raises(lib.X2HipError):
        K.sample_negatives(torch.zeros(1025, 1025, device=dev), torch.zeros(1025, device=dev))
    with pytest.raises(lib.X2HipError):
        K.gather_rows(torch.zeros(4, 6, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), 6)
    torch.cuda.synchronize()                                                                         # nothing was launched, nothing faulted
