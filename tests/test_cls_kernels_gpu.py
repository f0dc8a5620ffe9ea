"""The classification kernels (csrc/classify.hip) against float64 autograd of the reference expression
F.cross_entropy(Linear(GELU(LayerNorm(h, eps=1e-5))), labels, ignore_index=-100) - the tail of build_mlp (xvlm.py:163-169) and
model_classification.py's loss line - and x2_cls_accuracy against torch.

Metric and bound: relerr and slice_relerr (row by row) at 1e-5 of max-abs, the project's fp32 rule (tests/test_small_kernels_gpu.py), for every
output and every gradient.  Measured worst on the MI355X over all of them: 3.1e-6 (a row's logits at (257, 1028, 2)).

Shapes (R, H, C): (1, 4, 2) the smallest legal call; (2, 252, 2) and (3, 260, 3) one float4 short of / past a 256-thread trip and of the
64-column groups of the backward's second launch; (63, 256, 2), (64, 1024, 16), (65, 3072, 2) around the 64-row chunk that launch stages, with
the widest C; (64, 4096, 2) the NLVR head of X2VLM-large; (257, 1028, 2) five chunks and a partial column group.  Each with ldh = lddh = H and
H + 4, the pad columns of h holding NaN and those of dh guarded.
Rows are scaled 10^-1 .. 10^1 over the row index, and row R // 2 is moved to mean = 10 x its std (E[x^2] - E[x]^2 would lose the variance there).
Labels: all valid; -100 first; -100 last; all but one -100; NULL (nll and stat keep their sentinels).  A combination that leaves no valid row is
skipped (the loss is NaN there, as in torch; documented, not tested).  Cotangents: g_loss alone, g_logits alone, both.
Every output is written inside kernel_helpers.guarded sentinels, inputs sit in guarded copies, and a second run of each launch gives the same
bits.

x2_cls_accuracy: R in {1, 63, 64, 65, 257, 5000} x C in {2, 3, 16} against torch.argmax on well-separated logits and against the lowest index
of the row maximum on bit-equal logits (built by x2_cls_tail_fwd from duplicate w rows); counts accumulate over three launches."""
import importlib

import pytest
import torch
import torch.nn.functional as Fn

from kernel_helpers import F32, I32, I64, SENTINEL, filled, guarded, relerr, slice_relerr

pytestmark = pytest.mark.gpu
dev = "cuda"
TOL = 1e-5
EPS = 1e-5
SHAPES = [(1, 4, 2), (2, 252, 2), (3, 260, 3), (63, 256, 2), (64, 1024, 16), (65, 3072, 2), (64, 4096, 2), (257, 1028, 2)]
LABEL_MODES = ["valid", "first", "last", "one", "null"]
COTANGENTS = [(0.7, False), (None, True), (0.7, True)]


def _call(name, *args):
    lib = importlib.import_module("x2-vlm_amd._lib")
    lib.call(name, *[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args])


def check(name, got, ref, tol=TOL):
    ref = ref.reshape(got.shape) if ref.numel() == got.numel() else ref
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    whole = relerr(got, ref)
    sl = slice_relerr(got, ref) if got.dim() == 2 else whole
    print("%-64s relerr %.3e  slice_relerr %.3e  (bound %.0e)" % (name, whole, sl, tol))
    assert whole < tol and sl < tol, (name, whole, sl, tol)


def make_inputs(R, H, C, seed=0):
    g = torch.Generator().manual_seed(1000 * seed + 7 * R + H + C)
    scale = 10.0 ** torch.linspace(-1.0, 1.0, R) if R > 1 else torch.ones(1)
    h = torch.randn(R, H, generator=g) * scale[:, None]
    h[R // 2] += 10.0 * h[R // 2].std(unbiased=False)
    gamma = 1.0 + 0.2 * torch.randn(H, generator=g)
    beta = 0.2 * torch.randn(H, generator=g)
    w = torch.randn(C, H, generator=g) / H ** 0.5
    bias = 0.3 * torch.randn(C, generator=g)
    g_logits = torch.randn(R, C, generator=g)
    valid = torch.randint(0, C, (R,), generator=g)
    return h, gamma, beta, w, bias, g_logits, valid


def labels_of(mode, valid):
    R = valid.numel()
    lab = valid.clone()
    if mode == "null":
        return None
    if mode == "first":
        lab[0] = -100
    elif mode == "last":
        lab[R - 1] = -100
    elif mode == "one":
        lab[:] = -100
        lab[R // 3] = valid[R // 3]
    return lab if bool((lab >= 0).any()) else "skip"


class Reference:
    """float64 autograd of the reference expression on the (fp32) inputs"""

    def __init__(self, h, gamma, beta, w, bias, labels):
        self.leaves = [t.double().requires_grad_(True) for t in (h, gamma, beta, w, bias)]
        x, g, b, ww, bb = self.leaves
        self.mean = x.detach().mean(1)
        self.rstd = (x.detach().var(1, unbiased=False) + EPS).rsqrt()
        self.logits = Fn.linear(Fn.gelu(Fn.layer_norm(x, (x.shape[1],), g, b, EPS)), ww, bb)
        self.loss = self.nll = None
        if labels is not None:
            self.loss = Fn.cross_entropy(self.logits, labels, ignore_index=-100)
            self.nll = Fn.cross_entropy(self.logits.detach(), labels, ignore_index=-100, reduction="none")
            self.n_valid = int((labels >= 0).sum())

    def grads(self, g_loss, g_logits):
        total = 0.0
        if g_loss is not None:
            total = total + g_loss * self.loss
        if g_logits is not None:
            total = total + (g_logits.double() * self.logits).sum()
        return torch.autograd.grad(total, self.leaves, retain_graph=True)


class Device:
    """the inputs in guarded copies (pad columns of h: NaN), the forward's outputs inside guards"""

    def __init__(self, h, gamma, beta, w, bias, labels, ld):
        self.R, self.H = h.shape
        self.C = w.shape[0]
        self.ld = ld
        self.h, self.gamma, self.beta, self.w, self.bias = filled(h, ld=ld), filled(gamma), filled(beta), filled(w), filled(bias)
        self.labels = None if labels is None else filled(labels)
        self.guards = []

    def out(self, shape, dtype=F32, name="buffer", **kw):
        v, g = guarded(shape, dtype, name=name, **kw)
        self.guards.append(g)
        return v

    def forward(self):
        R, H, C = self.R, self.H, self.C
        o = dict(logits=self.out((R, C), name="logits"), rowstat=self.out((R, 2), name="rowstat"), nll=self.out((R,), name="nll"),
                 stat=self.out((2,), name="stat"))
        _call("x2_cls_tail_fwd", self.h, self.ld, self.gamma, self.beta, self.w, self.bias, self.labels, R, H, C, EPS, o["logits"], o["rowstat"],
              o["nll"], o["stat"])
        return o

    def backward(self, fwd, g_loss, g_logits):
        R, H, C = self.R, self.H, self.C
        o = dict(dh=self.out((R, H), ld=self.ld, name="dh"), dgamma=self.out((H,), name="dgamma"), dbeta=self.out((H,), name="dbeta"),
                 dw=self.out((C, H), name="dw"), dbias=self.out((C,), name="dbias"))
        _call("x2_cls_tail_bwd", self.h, self.ld, self.gamma, self.beta, self.w, fwd["rowstat"], fwd["logits"], self.labels,
              fwd["stat"] if self.labels is not None else None, g_loss, g_logits, R, H, C, o["dh"], self.ld, o["dgamma"], o["dbeta"], o["dw"],
              o["dbias"])
        return o

    def check_guards(self):
        torch.cuda.synchronize()
        for g in self.guards:
            g()


def untouched(t):
    return bool((t.view(I32) == SENTINEL[F32]).all())


@pytest.mark.parametrize("pad", [0, 4], ids=["ld=H", "ld=H+4"])
@pytest.mark.parametrize("R,H,C", SHAPES, ids=["%dx%dx%d" % s for s in SHAPES])
def test_cls_tail_matches_float64_autograd(R, H, C, pad):
    h, gamma, beta, w, bias, g_logits, valid = make_inputs(R, H, C)
    ran = 0
    for mode in LABEL_MODES:
        labels = labels_of(mode, valid)
        if isinstance(labels, str):
            continue
        tag = "cls_tail %dx%dx%d pad %d labels %-5s " % (R, H, C, pad, mode)
        ref = Reference(h, gamma, beta, w, bias, labels)
        d = Device(h, gamma, beta, w, bias, labels, H + pad)
        f = d.forward()
        f2 = d.forward()
        d.check_guards()
        check(tag + "logits", f["logits"], ref.logits)
        check(tag + "mean", f["rowstat"][:, :1], ref.mean)
        check(tag + "rstd", f["rowstat"][:, 1:], ref.rstd)
        assert torch.equal(f["logits"], f2["logits"]) and torch.equal(f["rowstat"], f2["rowstat"])
        if labels is None:
            assert untouched(f["nll"]) and untouched(f["stat"])
        else:
            check(tag + "nll", f["nll"].view(R, 1), ref.nll)
            check(tag + "loss", f["stat"][:1], ref.loss.detach().reshape(1))
            assert float(f["stat"][1]) == ref.n_valid
            assert bool((f["nll"][d.labels < 0] == 0).all())
            assert torch.equal(f["nll"], f2["nll"]) and torch.equal(f["stat"], f2["stat"])
        gl_dev = filled(g_logits)
        gs_dev = filled(torch.tensor([0.7]))
        for g_loss, with_logits in COTANGENTS:
            if labels is None and g_loss is not None:
                continue
            want = ref.grads(g_loss, g_logits if with_logits else None)
            args = (f, gs_dev if g_loss is not None else None, gl_dev if with_logits else None)
            b, b2 = d.backward(*args), d.backward(*args)
            d.check_guards()
            ctag = tag + "g_loss %s g_logits %d " % (g_loss, with_logits)
            for name, ref_g in zip(("dh", "dgamma", "dbeta", "dw", "dbias"), want):
                check(ctag + name, b[name], ref_g)
                assert torch.equal(b[name], b2[name]), name
            ran += 1
    assert ran >= 3


def test_ignored_rows_pass_only_the_logits_cotangent():
    """dlogits of an ignored row is g_logits alone: with g_loss alone its dh row is exactly zero"""
    R, H, C = 5, 64, 3
    h, gamma, beta, w, bias, g_logits, valid = make_inputs(R, H, C, seed=1)
    labels = valid.clone()
    labels[2] = -100
    d = Device(h, gamma, beta, w, bias, labels, H)
    f = d.forward()
    b = d.backward(f, filled(torch.tensor([1.0])), None)
    d.check_guards()
    assert bool((b["dh"][2] == 0).all()) and bool((b["dh"][[0, 1, 3, 4]].abs().amax(1) > 0).all())
    assert float(f["stat"][1]) == 4.0


SEP_R = [1, 63, 64, 65, 257, 5000]


@pytest.mark.parametrize("C", [2, 3, 16])
def test_cls_accuracy_matches_torch(C):
    for R in SEP_R:
        g = torch.Generator().manual_seed(R * 31 + C)
        logits = torch.randn(R, C, generator=g)
        labels = torch.randint(0, C, (R,), generator=g)
        if R > 2:
            labels[1] = -100                                             # never equal to a prediction, still counted
        lg, lb = filled(logits), filled(labels)
        pred, gp = guarded((R,), I32, name="pred")
        counts, gc = guarded((2,), I64, name="counts")
        counts.zero_()
        want = logits.argmax(1)
        for launch in range(1, 4):                                       # counts accumulate over launches on one stream
            _call("x2_cls_accuracy", lg, lb, R, C, pred, counts)
            torch.cuda.synchronize()
            assert counts.tolist() == [launch * int((want == labels).sum()), launch * R], (R, C, launch)
        gp(), gc()
        assert pred.dtype == I32 and torch.equal(pred.cpu().long(), want)


@pytest.mark.parametrize("C", [3, 16])
def test_cls_accuracy_takes_the_lowest_index_of_equal_maxima(C):
    """duplicate rows of w (and equal biases) give bit-equal logits; the strict > keeps the lowest index, prediction.max(1)'s rule"""
    R, H = 65, 256
    h, gamma, beta, w, bias, _, _ = make_inputs(R, H, C, seed=2)
    w[C - 1], bias[C - 1] = w[0], bias[0]
    if C > 3:
        w[2], bias[2] = w[1], bias[1]
    d = Device(h, gamma, beta, w, bias, None, H)
    logits = d.forward()["logits"]
    host = logits.cpu()
    assert torch.equal(host[:, C - 1], host[:, 0]) and (C == 3 or torch.equal(host[:, 2], host[:, 1]))
    first = (host == host.amax(1, keepdim=True)).int().argmax(1)         # the first index that holds the maximum
    assert bool(((host == host.amax(1, keepdim=True)).sum(1) >= 2).any()) and not bool((first == C - 1).any())
    labels = first.clone().long()
    labels[::2] = C - 1                                                  # column C - 1 repeats column 0 and is never the lowest index: counted wrong
    pred, gp = guarded((R,), I32, name="pred")
    counts, gc = guarded((2,), I64, name="counts")
    counts.zero_()
    _call("x2_cls_accuracy", logits, filled(labels), R, C, pred, counts)
    torch.cuda.synchronize()
    gp(), gc()
    assert torch.equal(pred.cpu().int(), first.int())
    assert counts.tolist() == [int((first == labels).sum()), R]
