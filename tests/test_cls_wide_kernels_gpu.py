"""csrc/classify_wide.hip against float64 torch autograd on the CPU: LayerNorm -> GELU (forward to bf16, backward), the cross-entropy with several
weighted targets per row, the KL divergence to a dense teacher, their bf16 dlogits, the row argmax / accuracy, and ops.cls_wide composed of them
and the GEMMs.

Shapes (R, H, C): (1, 64, 17), (2, 64, 63), (3, 128, 64), (5, 192, 65), (257, 256, 129), (65, 2048, 1000), (64, 1536, 3129) - one row, C below /
at / above the padding unit 64 and no multiple of 4, more rows than one workgroup walks at once, the two real head widths.  Every shape runs with
the minimal leading dimensions and with + 4 (ldl = C is odd for most shapes: scalar row reads; C + 4 with C % 4 == 0 the float4 path); every input
sits in a buffer whose other elements - the columns beyond C or H, the gap between rows, what lies before and behind - are NaN, so a read outside
[0, C) poisons the result; every output and workspace lies between kernel_helpers.Guard sentinels.
Entries: rows take k = 1, 0, 37 in turn (row 4 of the five-row shape 300: more than one staged chunk of 256), every fifth entry of a row is -100,
entries 3 and 4 of a long row repeat entry 2's target; weights NULL and given; denom_mode 0 and 1; also T = 0 for the whole batch.
Cotangents: g_loss alone, g_logits alone, both.  Teacher rows are scaled by up to 60, so that exp(t - lse_t) underflows for many columns.
Rows of h are scaled by 10^-1 .. 10^1 and the last row's mean is 10 x its standard deviation.

Bounds.  fp32 outputs (lse, rowloss, stat, rowstat, dh, dgamma, dbeta): 1e-5 of the reference's max-abs, for the whole tensor and row by row
(tests/test_cls_kernels_gpu.py's bound for the same class of arithmetic).  bf16 outputs (act, dl): within one bf16 ulp of the float64 value
rounded to bf16; for dl, a sum of fp32 terms that may cancel, plus the rounding of that sum's own operands, 2^-20 x (|g_logits| + |scale Wr
softmax| + |scale sum w|), which no fp32 evaluation can avoid; pad columns exactly 0.
Composed ops.cls_wide (logits, loss, dW, dbias, dh) against a float64 reference whose operands are rounded to bf16 where the path rounds them (act,
W, dl), relative to each tensor's max-abs: measured worst over the seven shapes and both losses 2.24e-5 (dW at 64 x 1536 x 3129, where a handful
of act / dl elements round to the neighbouring bf16 number; logits 6.62e-6 there; every other tensor and shape below 1.1e-6; printed below).
Bound 1.5 x the worst, rounded up: 3.4e-5."""
import importlib
import math

import pytest
import torch

from kernel_helpers import BF16, F32, I32, I64, K, dev, filled, guarded, lib, relerr, rowerr  # noqa: F401  (K, lib: fixtures)

pytestmark = pytest.mark.gpu
raw = importlib.import_module("x2-vlm_amd._lib")
SHAPES = [(1, 64, 17), (2, 64, 63), (3, 128, 64), (5, 192, 65), (257, 256, 129), (65, 2048, 1000), (64, 1536, 3129)]
IDS = ["%dx%dx%d" % s for s in SHAPES]
F32_BOUND = 1e-5
COMPOSED_BOUND = 3.4e-5
EPS = 1e-5


def rup(x, m):
    return (x + m - 1) // m * m


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ulp_bf16(v):
    """one unit in the last place of the bf16 number v (float64 tensor): 2^(floor(log2 |v|) - 7), the smallest normal's for 0 and subnormals"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), (e - 8).double())


def to_bf16_64(x64):
    return x64.float().to(BF16).double()


def check_f32(name, got, ref, rows=True):
    e = relerr(got, ref)
    er = 0.0
    if rows and ref.numel() > 2:                      # a vector of per-row results: element by element
        er = rowerr(got.reshape(ref.shape[0], -1), ref.reshape(ref.shape[0], -1))
    print("  %-10s max-abs relative error %.2e, worst row %.2e (bound %.0e)" % (name, e, er, F32_BOUND))
    assert e <= F32_BOUND and er <= F32_BOUND, (name, e, er)


def check_bf16(name, got, ref64, floor=None):
    """got bf16 [R, n] within one bf16 ulp (+ floor) of ref64 rounded to bf16"""
    want = to_bf16_64(ref64)
    g = got.detach().cpu().double()
    assert bool(torch.isfinite(g).all()), name
    tol = ulp_bf16(want) + (0.0 if floor is None else floor)
    over = (g - want).abs() - tol
    print("  %-10s bf16: %d of %d elements differ from the rounded reference, worst excess over the tolerance %.2e"
          % (name, int((g != want).sum()), g.numel(), float(over.max())))
    assert bool((over <= 0).all()), (name, float(over.max()))


def same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ inputs and float64 references

def head_inputs(R, H, seed=1):
    g = gen(seed)
    h = torch.randn(R, H, generator=g) * torch.pow(10.0, torch.rand(R, 1, generator=g) * 2 - 1)
    h[R - 1] += 10.0 * h[R - 1].std()                                        # a row whose mean is 10 x its standard deviation
    gamma = 1.0 + 0.1 * torch.randn(H, generator=g)
    beta = 0.1 * torch.randn(H, generator=g)
    return h, gamma, beta


def ref_lngelu(h, gamma, beta):
    h = h.double()
    mean = h.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((h - mean) ** 2).mean(1, keepdim=True) + EPS)
    y = (h - mean) * rstd * gamma.double() + beta.double()
    return 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0))), mean, rstd


def entries(R, C, seed=2, empty=False):
    """(k list, offs int32 [R + 1], targets int64 [T], weights fp32 [T])"""
    g = gen(seed)
    k = [0] * R if empty else [(300 if (R == 5 and r == 4) else (1, 0, 37)[r % 3]) for r in range(R)]
    tg = []
    for kr in k:
        t = torch.randint(0, C, (kr,), generator=g)
        if kr >= 5:
            t[3] = t[4] = t[2]
        t[torch.arange(kr) % 5 == 0] = -100
        if kr == 1:
            t[0] = int(torch.randint(0, C, (1,), generator=g))               # single entries stay valid: some rows must count
        tg.append(t)
    targets = torch.cat(tg) if tg else torch.zeros(0, dtype=I64)
    offs = torch.tensor([0] + list(torch.tensor(k).cumsum(0)), dtype=I32)
    weights = torch.randint(1, 11, (targets.numel(),), generator=g).float() / 10.0
    return k, offs, targets.to(I64), weights


def ref_soft_ce(z, k, targets, weights, denom_mode, g_loss, g_logits):
    """float64: (lse, rowloss, stat, dl, operand magnitude of dl's sum)"""
    z = z.double().requires_grad_(True)
    R, C = z.shape
    lse = torch.logsumexp(z, 1)
    row = torch.repeat_interleave(torch.arange(R), torch.tensor(k, dtype=I64))
    valid = (targets >= 0) & (targets < C)
    w = torch.ones(targets.numel(), dtype=torch.float64) if weights is None else weights.double()
    w = torch.where(valid, w, torch.zeros_like(w))
    tt = targets.clamp(0, C - 1)
    rowloss = torch.zeros(R, dtype=torch.float64).index_add(0, row, w * (lse[row] - z[row, tt]))
    wr = torch.zeros(R, dtype=torch.float64).index_add(0, row, w)
    sub = torch.zeros(R, C, dtype=torch.float64).index_put((row, tt), w, accumulate=True)
    n = int(valid.sum())
    denom = float(R) if denom_mode == 0 else float(n)
    loss = rowloss.sum() / denom
    total = torch.zeros((), dtype=torch.float64)
    if g_loss is not None:
        total = total + float(g_loss) * loss
    if g_logits is not None:
        total = total + (g_logits.double() * z).sum()
    (dl,) = torch.autograd.grad(total, z)
    scale = 0.0 if g_loss is None else abs(float(g_loss)) / denom
    mag = scale * (wr[:, None] * torch.softmax(z.detach(), 1) + sub) + (0.0 if g_logits is None else g_logits.double().abs())
    return lse.detach(), rowloss.detach(), torch.tensor([float(loss), denom], dtype=torch.float64), dl, mag


def ref_kl(z, t, g_loss, g_logits):
    z = z.double().requires_grad_(True)
    t = t.double()
    R = z.shape[0]
    lse, lse_t = torch.logsumexp(z, 1), torch.logsumexp(t, 1)
    p = torch.exp(t - lse_t[:, None])
    rowloss = torch.where(p > 0, p * ((t - lse_t[:, None]) - (z - lse[:, None])), torch.zeros_like(p)).sum(1)
    loss = rowloss.sum() / R
    total = torch.zeros((), dtype=torch.float64)
    if g_loss is not None:
        total = total + float(g_loss) * loss
    if g_logits is not None:
        total = total + (g_logits.double() * z).sum()
    (dl,) = torch.autograd.grad(total, z)
    scale = 0.0 if g_loss is None else abs(float(g_loss)) / R
    mag = scale * (torch.softmax(z.detach(), 1) + p) + (0.0 if g_logits is None else g_logits.double().abs())
    return lse.detach(), lse_t, rowloss.detach(), torch.tensor([float(loss), float(R)], dtype=torch.float64), dl, mag


def nan_rows(t, pad):
    """device copy of host [R, n] rows, pad elements apart beyond n, NaN everywhere else"""
    return filled(t.contiguous(), ld=t.shape[1] + pad)


def padded_dl(R, C, pad):
    Cp = rup(C, 64)
    dl, guard = guarded((R, Cp), BF16, ld=Cp + pad, name="dl")
    return dl, guard, Cp


COTANGENTS = [("loss", True, False), ("logits", False, True), ("both", True, True)]


# ------------------------------------------------------------------------------------------------------------------ LayerNorm -> GELU

@pytest.mark.parametrize("pad", [0, 4], ids=["ld_min", "ld+4"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_lngelu_forward_and_backward(shape, pad):
    R, H, _ = shape
    h, gamma, beta = head_inputs(R, H)
    act_ref, mean, rstd = ref_lngelu(h, gamma, beta)
    hd, gd, bd = nan_rows(h, pad), filled(gamma), filled(beta)
    outs = []
    for _ in range(2):
        act, g_act = guarded((R, H), BF16, ld=H + pad, name="act")
        rowstat, g_rs = guarded((R, 2), F32, name="rowstat")
        raw.call("x2_lngelu_fwd", hd.data_ptr(), hd.stride(0), gd.data_ptr(), bd.data_ptr(), R, H, EPS, act.data_ptr(), act.stride(0), rowstat.data_ptr())
        torch.cuda.synchronize()
        g_act(), g_rs()
        outs.append((act.clone(), rowstat.clone()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    print("lngelu %s ld+%d" % (shape, pad))
    check_bf16("act", outs[0][0], act_ref)
    # {mean, rstd} column by column: the two live on different scales
    check_f32("mean", outs[0][1][:, 0], mean[:, 0], rows=False)          # row by row: below, every row to its own scale
    check_f32("rstd", outs[0][1][:, 1], rstd[:, 0])
    assert float(((outs[0][1][:, 0].cpu().double() - mean[:, 0]).abs() / h.double().abs().amax(1)).max()) <= F32_BOUND      # every row to its own scale
    assert float(((outs[0][1][:, 1].cpu().double() - rstd[:, 0]).abs() / rstd[:, 0]).max()) <= F32_BOUND

    # backward: float64 autograd of sum(dact * gelu(LN(h)))
    dact = torch.randn(R, H, generator=gen(3))
    h64, g64, b64 = h.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m = h64.mean(1, keepdim=True)
    y = (h64 - m) / torch.sqrt(((h64 - m) ** 2).mean(1, keepdim=True) + EPS) * g64 + b64
    (0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0))) * dact.double()).sum().backward()
    dd = nan_rows(dact, pad)
    rs = filled(torch.cat([mean, rstd], 1).float())
    outs = []
    for _ in range(2):
        dh, g_dh = guarded((R, H), F32, ld=H + pad, name="dh")
        dg, g_dg = guarded((H,), F32, name="dgamma")
        db, g_db = guarded((H,), F32, name="dbeta")
        raw.call("x2_lngelu_bwd", dd.data_ptr(), dd.stride(0), hd.data_ptr(), hd.stride(0), gd.data_ptr(), bd.data_ptr(), rs.data_ptr(), R, H,
                 dh.data_ptr(), dh.stride(0), dg.data_ptr(), db.data_ptr())
        torch.cuda.synchronize()
        g_dh(), g_dg(), g_db()
        outs.append((dh.clone(), dg.clone(), db.clone()))
    assert all(same_bits(a, b) for a, b in zip(*outs))
    check_f32("dh", outs[0][0], h64.grad)
    check_f32("dgamma", outs[0][1], g64.grad, rows=False)                 # column sums: one row each
    check_f32("dbeta", outs[0][2], b64.grad, rows=False)


# ------------------------------------------------------------------------------------------------------------------ soft cross-entropy

def run_soft_ce(z_d, R, C, offs, targets, weights, mode, pad, g_loss=None, g_logits=None, want_bwd=True):
    """raw launches with guarded outputs -> dict of clones (every guard checked)"""
    od = filled(offs)
    td = filled(targets) if targets.numel() else filled(torch.full((1,), -100, dtype=I64))
    wd = None if weights is None else (filled(weights) if weights.numel() else filled(torch.zeros(1)))
    lse, g1 = guarded((R,), F32, name="lse")
    rowloss, g2 = guarded((R,), F32, name="rowloss")
    stat, g3 = guarded((2,), F32, name="stat")
    raw.call("x2_soft_ce_fwd", z_d.data_ptr(), z_d.stride(0), R, C, od.data_ptr(), td.data_ptr(), raw.ptr(wd), mode, lse.data_ptr(),
             rowloss.data_ptr(), stat.data_ptr())
    torch.cuda.synchronize()
    g1(), g2(), g3()
    out = dict(lse=lse.clone(), rowloss=rowloss.clone(), stat=stat.clone())
    if want_bwd:
        gl = None if g_loss is None else filled(torch.tensor([g_loss], dtype=F32))
        gz = None if g_logits is None else nan_rows(g_logits, pad)
        dl, g4, Cp = padded_dl(R, C, pad)
        raw.call("x2_soft_ce_bwd", z_d.data_ptr(), z_d.stride(0), R, C, od.data_ptr(), td.data_ptr(), raw.ptr(wd), lse.data_ptr(), stat.data_ptr(),
                 raw.ptr(gl), raw.ptr(gz), 0 if gz is None else gz.stride(0), dl.data_ptr(), dl.stride(0), Cp)
        torch.cuda.synchronize()
        g4()
        out["dl"] = dl.clone()
    return out


@pytest.mark.parametrize("pad", [0, 4], ids=["ld_min", "ld+4"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_soft_ce_forward_and_backward(shape, pad):
    R, _, C = shape
    z = torch.randn(R, C, generator=gen(4)) * 2.0
    z_d = nan_rows(z, pad)
    k, offs, targets, weights = entries(R, C)
    g_logits = torch.randn(R, C, generator=gen(5)) * 1e-2
    print("soft_ce %s ld+%d: T = %d, %d ignored" % (shape, pad, targets.numel(), int((targets < 0).sum())))
    for mode, w in ((0, weights), (1, None), (1, weights), (0, None)):
        for cname, use_gl, use_gz in (COTANGENTS if (mode, w is None) in ((0, False), (1, True)) else COTANGENTS[2:]):
            gl, gz = (0.7 if use_gl else None), (g_logits if use_gz else None)
            lse, rowloss, stat, dl, mag = ref_soft_ce(z, k, targets, w, mode, gl, gz)
            a = run_soft_ce(z_d, R, C, offs, targets, w, mode, pad, gl, gz)
            b = run_soft_ce(z_d, R, C, offs, targets, w, mode, pad, gl, gz)
            assert all(same_bits(a[n], b[n]) for n in a), "two runs differ"
            print(" denom_mode %d, weights %s, cotangent %s" % (mode, "NULL" if w is None else "given", cname))
            check_f32("lse", a["lse"], lse)
            check_f32("rowloss", a["rowloss"], rowloss)
            check_f32("stat", a["stat"], stat)
            assert float(a["stat"][1]) == float(stat[1])
            Cp = a["dl"].shape[1]
            check_bf16("dl", a["dl"][:, :C], dl, floor=2.0 ** -20 * mag)
            assert Cp % 64 == 0 and bool((a["dl"][:, C:] == 0).all()), "pad columns of dl must be exactly 0"


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[4]], ids=[IDS[1], IDS[4]])
def test_soft_ce_without_any_entry(shape):
    """T = 0 for the whole batch: rowloss 0, loss 0 over R rows, dl = g_logits alone"""
    R, _, C = shape
    z = torch.randn(R, C, generator=gen(6))
    g_logits = torch.randn(R, C, generator=gen(7))
    k, offs, targets, weights = entries(R, C, empty=True)
    assert targets.numel() == 0 and int(offs[-1]) == 0
    a = run_soft_ce(nan_rows(z, 0), R, C, offs, targets, weights, 0, 0, 0.7, g_logits)
    assert bool((a["rowloss"] == 0).all()) and float(a["stat"][0]) == 0.0 and float(a["stat"][1]) == R
    check_f32("lse", a["lse"], torch.logsumexp(z.double(), 1))
    check_bf16("dl", a["dl"][:, :C], g_logits.double())
    assert bool((a["dl"][:, C:] == 0).all())


def test_no_loss_asked_for_leaves_rowloss_and_stat_alone(K):
    """targets NULL: only lse is written, the sentinels of rowloss and stat stay; g_loss NULL: dl is bf16(g_logits), the loss's tensors unread"""
    R, C = 5, 65
    z = torch.randn(R, C, generator=gen(8))
    z_d = nan_rows(z, 4)
    od = filled(torch.arange(R + 1, dtype=I32))
    lse, g1 = guarded((R,), F32, name="lse")
    rowloss, g2 = guarded((R,), F32, name="rowloss")
    stat, g3 = guarded((2,), F32, name="stat")
    raw.call("x2_soft_ce_fwd", z_d.data_ptr(), z_d.stride(0), R, C, od.data_ptr(), None, None, 0, lse.data_ptr(), rowloss.data_ptr(), stat.data_ptr())
    torch.cuda.synchronize()
    g1(), g2(), g3()
    check_f32("lse", lse, torch.logsumexp(z.double(), 1))
    assert bool(torch.isnan(rowloss).all()) and bool(torch.isnan(stat).all())                 # still the NaN sentinel
    assert bool((rowloss.view(I32) == 0x7FC5A5A5).all()) and bool((stat.view(I32) == 0x7FC5A5A5).all())
    g_logits = torch.randn(R, C, generator=gen(9))
    for entry in ("x2_soft_ce_bwd", "x2_kl_ce_bwd"):
        dl, g4, Cp = padded_dl(R, C, 4)
        gz = nan_rows(g_logits, 0)
        if entry == "x2_soft_ce_bwd":
            raw.call(entry, None, 0, R, C, None, None, None, None, None, None, gz.data_ptr(), gz.stride(0), dl.data_ptr(), dl.stride(0), Cp)
        else:
            raw.call(entry, None, 0, None, 0, R, C, None, None, None, gz.data_ptr(), gz.stride(0), dl.data_ptr(), dl.stride(0), Cp)
        torch.cuda.synchronize()
        g4()
        assert torch.equal(dl[:, :C].cpu(), g_logits.to(BF16)) and bool((dl[:, C:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ KL to a dense teacher

@pytest.mark.parametrize("pad", [0, 4], ids=["ld_min", "ld+4"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kl_forward_and_backward(shape, pad):
    R, _, C = shape
    z = torch.randn(R, C, generator=gen(10)) * 2.0
    t = torch.randn(R, C, generator=gen(11)) * torch.linspace(1.0, 60.0, R)[:, None]        # the sharp rows' small p_c underflow to 0
    g_logits = torch.randn(R, C, generator=gen(12)) * 1e-2
    z_d, t_d = nan_rows(z, pad), nan_rows(t, pad)
    p = torch.softmax(t.double(), 1).float()
    print("kl %s ld+%d: %d of %d teacher probabilities underflow in fp32" % (shape, pad, int((p == 0).sum()), p.numel()))
    assert R < 3 or bool((p == 0).any())
    for cname, use_gl, use_gz in COTANGENTS:
        gl, gz = (0.7 if use_gl else None), (g_logits if use_gz else None)
        lse, lse_t, rowloss, stat, dl, mag = ref_kl(z, t, gl, gz)
        outs = []
        for _ in range(2):
            bufs = [guarded((R,), F32, name=n) for n in ("lse", "lse_t", "rowloss")] + [guarded((2,), F32, name="stat")]
            raw.call("x2_kl_ce_fwd", z_d.data_ptr(), z_d.stride(0), t_d.data_ptr(), t_d.stride(0), R, C, *[b.data_ptr() for b, _ in bufs])
            gld = None if gl is None else filled(torch.tensor([gl], dtype=F32))
            gzd = None if gz is None else nan_rows(gz, pad)
            d, g4, Cp = padded_dl(R, C, pad)
            raw.call("x2_kl_ce_bwd", z_d.data_ptr(), z_d.stride(0), t_d.data_ptr(), t_d.stride(0), R, C, bufs[0][0].data_ptr(), bufs[1][0].data_ptr(),
                     raw.ptr(gld), raw.ptr(gzd), 0 if gzd is None else gzd.stride(0), d.data_ptr(), d.stride(0), Cp)
            torch.cuda.synchronize()
            for _, g in bufs:
                g()
            g4()
            outs.append([b.clone() for b, _ in bufs] + [d.clone()])
        assert all(same_bits(a, b) for a, b in zip(*outs)), "two runs differ"
        print(" cotangent %s" % cname)
        for name, got, ref in zip(("lse", "lse_t", "rowloss", "stat"), outs[0], (lse, lse_t, rowloss, stat)):
            check_f32(name, got, ref)
        check_bf16("dl", outs[0][4][:, :C], dl, floor=2.0 ** -20 * mag)
        assert bool((outs[0][4][:, C:] == 0).all()), "pad columns of dl must be exactly 0"


# ------------------------------------------------------------------------------------------------------------------ accuracy

@pytest.mark.parametrize("C", [17, 64, 65, 3129])
@pytest.mark.parametrize("R", [1, 63, 65, 5000])
def test_accuracy_rows_is_argmax_with_the_lowest_index(R, C):
    g = gen(13 + R + C)
    z = (torch.randn(R, C, generator=g) * 2.0).round() / 2.0                  # a coarse grid: many rows' maxima are shared by several columns,
    even = torch.arange(0, R, 2)                                               # and every other row gets a bit-equal copy of its maximum
    z[even, torch.randint(0, C, (even.numel(),), generator=g)] = z[even].amax(1)
    ties = int(((z == z.amax(1, keepdim=True)).sum(1) > 1).sum())
    assert ties >= R // 3
    want = torch.argmax(z, 1)
    assert bool((want == (z == z.amax(1, keepdim=True)).float().argmax(1)).all())             # torch's argmax takes the first maximum
    labels = torch.where(torch.rand(R, generator=g) < 0.5, want, torch.randint(0, C, (R,), generator=g))
    labels[torch.arange(R) % 7 == 3] = -100                                   # a miss, whatever the prediction
    hits = int((labels == want).sum())
    pad = {17: 0, 64: 4, 65: 3, 3129: 2}[C]                                    # ld 17 and 3131: scalar rows; 68 and 68: float4 rows
    z_d, l_d = nan_rows(z, pad), filled(labels)
    counts, g_c = guarded((2,), I64, name="counts")
    counts.zero_()
    runs = []
    for _ in range(3):
        pred, g_p = guarded((R,), I32, name="pred")
        hit, g_h = guarded((R,), I32, name="hit")
        raw.call("x2_cls_accuracy_rows", z_d.data_ptr(), z_d.stride(0), l_d.data_ptr(), R, C, pred.data_ptr(), hit.data_ptr(), counts.data_ptr())
        torch.cuda.synchronize()
        g_p(), g_h(), g_c()
        runs.append((pred.clone(), hit.clone()))
    assert all(same_bits(runs[0][0], r[0]) and same_bits(runs[0][1], r[1]) for r in runs[1:])
    assert torch.equal(runs[0][0].cpu().long(), want), "%d rows with ties" % ties
    assert torch.equal(runs[0][1].cpu().long(), (labels == want).long())
    assert counts.tolist() == [3 * hits, 3 * R]
    assert not bool(runs[0][1].cpu()[labels == -100].any())


def test_accuracy_class_accumulates_over_batches(K):
    mcl = importlib.import_module("x2-vlm_amd.model_classification")
    acc = mcl.ClassificationAccuracy()
    total = correct = 0
    for i, R in enumerate((4, 33)):
        wide = torch.randn(R, 1536, generator=gen(40 + i)).to(dev)
        z = wide[:, :1500]                                                    # a column view of wider rows, as ops.cls_wide returns it
        want = torch.argmax(z, 1)
        labels = torch.where(torch.arange(R, device=dev) % 2 == 0, want, torch.full_like(want, -100))
        pred = acc.update(z, labels)
        assert pred.dtype == I32 and torch.equal(pred.long(), want)
        total, correct = total + R, correct + (R + 1) // 2
    assert acc.result() == {"acc": correct / total} and acc.formatted() == {"acc": "{:.4f}".format(correct / total)}


# ------------------------------------------------------------------------------------------------------------------ ops.cls_wide, composed

@pytest.mark.parametrize("loss_kind", ["soft", "kl"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_composed_cls_wide_against_bf16_rounded_float64(shape, loss_kind):
    ops = importlib.import_module("x2-vlm_amd.ops")
    xv = importlib.import_module("x2-vlm_amd.xvlm")
    R, H, C = shape
    h, gamma, beta = head_inputs(R, H, seed=20)
    g = gen(21)
    W, bias = torch.randn(C, H, generator=g) / math.sqrt(H), 0.1 * torch.randn(C, generator=g)
    seq = xv.build_mlp(H // 2, C)
    with torch.no_grad():
        seq[1].weight.copy_(gamma), seq[1].bias.copy_(beta), seq[3].weight.copy_(W), seq[3].bias.copy_(bias)
    seq = seq.to(dev)
    k, offs, targets, weights = entries(R, C, seed=22)
    teacher = torch.randn(R, C, generator=gen(23)) * 3.0
    g_logits = torch.randn(R, C, generator=gen(24)) * 1e-2
    hd = h.to(dev).requires_grad_(True)
    if loss_kind == "soft":
        logits, loss = ops.cls_wide(seq, hd, targets=targets.to(dev), offs=offs.to(dev), weights=weights.to(dev), denom_mode=0)
    else:
        logits, loss = ops.cls_wide(seq, hd, teacher=teacher.to(dev))
    assert logits.shape == (R, C) and logits.dtype == F32 and loss.dim() == 0
    (0.7 * loss + (logits * g_logits.to(dev)).sum()).backward()
    torch.cuda.synchronize()

    # float64, rounded where the path rounds: act and W before the logits GEMM, dl before the three gradient GEMMs / sums
    h64, g64, b64 = h.double().requires_grad_(True), gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    m = h64.mean(1, keepdim=True)
    y = (h64 - m) / torch.sqrt(((h64 - m) ** 2).mean(1, keepdim=True) + EPS) * g64 + b64
    act = 0.5 * y * (1.0 + torch.erf(y / math.sqrt(2.0)))
    act_b, W_b = to_bf16_64(act.detach()), to_bf16_64(W.double())
    z = act_b @ W_b.t() + bias.double()
    if loss_kind == "soft":
        _, _, stat, dl, _ = ref_soft_ce(z, k, targets, weights, 0, 0.7, g_logits)
    else:
        _, _, _, stat, dl, _ = ref_kl(z, teacher, 0.7, g_logits)
    dl_b = to_bf16_64(dl)
    act.backward(dl_b @ W_b)
    ref = dict(logits=z, loss=stat[0], dW=dl_b.t() @ act_b, dbias=dl_b.sum(0), dh=h64.grad, dgamma=g64.grad, dbeta=b64.grad)
    got = dict(logits=logits.detach(), loss=loss.detach(), dW=seq[3].weight.grad, dbias=seq[3].bias.grad, dh=hd.grad, dgamma=seq[1].weight.grad,
               dbeta=seq[1].bias.grad)
    errs = {n: relerr(got[n], ref[n]) for n in ref}
    print("cls_wide %s %s: " % (shape, loss_kind) + ", ".join("%s %.2e" % kv for kv in errs.items()) + " (bound %.1e)" % COMPOSED_BOUND)
    assert all(e <= COMPOSED_BOUND for e in errs.values()), errs


def test_cls_wide_refuses_a_width_the_gemm_cannot_contract():
    ops = importlib.import_module("x2-vlm_amd.ops")
    xv = importlib.import_module("x2-vlm_amd.xvlm")
    seq = xv.build_mlp(48, 100).to(dev)                                        # H = 96: a multiple of 4, not of 64
    with pytest.raises(ValueError, match="multiple of 64"):
        ops.cls_wide(seq, torch.zeros(4, 96, device=dev))
