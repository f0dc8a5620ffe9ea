"""GPU truth tests of the counter-based dropout inside the attention kernels (x2_attn_fwd / x2_attn_bwd) and inside the NT GEMM epilogue
(x2_gemm_nt), against float64 references that apply the SAME mask through the bit-exact host mirror kernels.dropout_keep().

keep(element) is regenerated in every kernel of a site from the element index, never stored: attention uses
((b*H + h)*Lq + q) * round_up(Lk, 64) + key, the GEMM epilogue m*N + n.  A kernel that lands on another index still trains and still agrees with
a sibling kernel making the same mistake; only a reference holding the mirrored mask sees it.  Every dispatch branch of x2_attn_fwd / x2_attn_bwd that
reads the dropout spec has a case here (the reached kernels are named per case), the GEMM feature sets run on all twelve pinned tile variants.

Tolerances are the project's own.  Attention (relative to max-abs, whole tensor and per (sequence, head) slice with a 5 % floor): Out 8e-3; dQ, dK,
dV and the batch-summed dS 1.5e-2 (P and dS are rounded to bf16 before the second MFMA).  GEMM: fp32-out 1e-5 per row, bf16-out 6e-3.
The "teeth" tests hold the device results at least 10 x those tolerances AWAY from two mutated references (mask shifted by one key; row pitch Lk
in place of round_up(Lk, 64)).  On the host, in float64 alone, the true and the mutated references of the three teeth geometries differ by
0.58 - 0.90 of max-abs on Out and 0.64 - 1.09 on dV, i.e. 70 x the tolerance and more.

Every attention test prints its worst error per tensor (run with -s).  Device figures have not been recorded here yet: this file was written
without a run on an MI355X, so a first run that misses a tolerance is a finding about the kernel (or about a case's dispatch comment), to be
traced in csrc/, not a reason to move a bound."""
import importlib

import pytest
import torch

from kernel_helpers import K, bf, nt_tile, nt_tile128, relerr, rnd, rowerr, slice_relerr, tuned  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
dev = "cuda"
TOL_OUT, TOL_GRAD = 8e-3, 1.5e-2


def _lib():
    return importlib.import_module("x2-vlm_amd._lib").lib()


# ------------------------------------------------------------------------------------------------ attention

class AttnCase:
    """One attention problem: bf16-rounded operands on the host, a float64 reference for a given keep tensor, and the device calls.
    Nothing touches the device until forward() / backward() is called (the mutated references are compared on the CPU alone)."""
    d = 64

    def __init__(self, K, B, Bkv, H, Lq, Lk, use_bias=False, use_mask=False, kv_map=None, seed=0, bias_log2=False):
        self.K, self.B, self.Bkv, self.H, self.Lq, self.Lk = K, B, Bkv, H, Lq, Lk
        self.kv_map, self.bias_log2, self.scale = kv_map, bias_log2, self.d ** -0.5
        D = H * self.d
        self.q, self.do = bf(rnd(B, Lq, D, seed=seed)), bf(rnd(B, Lq, D, seed=seed + 3))
        self.k, self.v = bf(rnd(Bkv, Lk, D, seed=seed + 1)), bf(rnd(Bkv, Lk, D, seed=seed + 2))
        self.bias = rnd(H, Lq, Lk, seed=seed + 4) if use_bias else None
        self.mask = None
        if use_mask:
            keep = (torch.rand(B, Lk, generator=torch.Generator().manual_seed(seed + 5)) > 0.3).float()
            keep[:, 0] = 1
            self.mask = (1 - keep) * -10000.0
        self.Lkp = K.round_up(Lk, 64)
        self._dev = None

    def index(self, pitch=None, shift=0):
        """dropout element index of every (sequence, head, query, key): int64 [B, H, Lq, Lk]"""
        B, H, Lq, Lk = self.B, self.H, self.Lq, self.Lk
        row = (torch.arange(B).view(B, 1, 1, 1) * H + torch.arange(H).view(1, H, 1, 1)) * Lq + torch.arange(Lq).view(1, 1, Lq, 1)
        return row * (self.Lkp if pitch is None else pitch) + torch.arange(Lk).view(1, 1, 1, Lk) + shift

    def reference(self, keep):
        """float64: O = (softmax(q k^T scale + bias + mask) * keep) v - the normalisation uses the undropped sum - and autograd's gradients for dO"""
        B, Bkv, H, Lq, Lk, d = self.B, self.Bkv, self.H, self.Lq, self.Lk, self.d
        heads = lambda t, B_, L_: t.double().view(B_, L_, H, d).permute(0, 2, 1, 3).clone().requires_grad_(True)
        q, k, v = heads(self.q, B, Lq), heads(self.k, Bkv, Lk), heads(self.v, Bkv, Lk)
        idx = torch.tensor(self.kv_map) if self.kv_map is not None else torch.arange(B)
        s = q @ k[idx].transpose(-1, -2) * self.scale
        bias = None
        if self.bias is not None:
            bias = self.bias.double().requires_grad_(True)
            s = s + bias.unsqueeze(0)
        if self.mask is not None:
            s = s + self.mask.double()[:, None, None, :]
        o = (torch.softmax(s, -1) * keep.double()) @ v[idx]
        o.backward(self.do.double().view(B, Lq, H, d).permute(0, 2, 1, 3))
        back = lambda t, B_, L_: t.detach().permute(0, 2, 1, 3).reshape(B_, L_, H * d)
        return dict(out=back(o, B, Lq), dq=back(q.grad, B, Lq), dk=back(k.grad, Bkv, Lk), dv=back(v.grad, Bkv, Lk),
                    dS=bias.grad if bias is not None else None)

    def reference_for(self, spec, **index_kw):
        return self.reference(self.K.dropout_keep(spec, self.index(**index_kw)))

    # ---- device ----
    def _device(self):
        if self._dev is not None:
            return self._dev
        K, B, Bkv, H, Lq, Lk, Lkp = self.K, self.B, self.Bkv, self.H, self.Lq, self.Lk, self.Lkp
        kw = {}
        if self.bias is not None:
            Lqp = K.round_up(Lq, 128 if Lq > 208 else 64)
            bp = torch.zeros(H, Lq, Lkp); bp[:, :, :Lk] = self.bias
            bT = torch.zeros(H, Lk, Lqp); bT[:, :, :Lq] = self.bias.transpose(1, 2)
            if self.bias_log2:            # the bias in log2 units, as kernels.relpos_bias(log2=True) hands it over
                bp, bT = bp * K.LOG2E, bT * K.LOG2E
                kw["bias_log2"] = True
            kw.update(bias=bp.to(dev), biasT=bT.to(dev))
        if self.mask is not None:
            mp = torch.zeros(B, Lkp); mp[:, :Lk] = self.mask
            kw["mask"] = mp.to(dev)
        if self.kv_map is not None:
            kv_idx = torch.tensor(self.kv_map, dtype=torch.int32)
            off = torch.zeros(Bkv + 1, dtype=torch.int32); off[1:] = torch.cumsum(torch.bincount(kv_idx, minlength=Bkv), 0)
            kw.update(kv_idx=kv_idx.to(dev), seq_off=off.to(dev), seq_ids=torch.argsort(kv_idx, stable=True).to(torch.int32).to(dev))
        t = {n: getattr(self, n).reshape(-1, H * self.d).to(dev) for n in ("q", "k", "v", "do")}
        self._dev = (kw, t)
        return self._dev

    def forward(self, spec):
        K, B, Bkv, H, Lq, Lk = self.K, self.B, self.Bkv, self.H, self.Lq, self.Lk
        kw, t = self._device()
        od = torch.full_like(t["q"], float("nan"))
        lse = torch.full((B * H * Lq,), float("nan"), device=dev)
        K.attn_fwd(K.view3(t["q"], B, Lq), K.view3(t["k"], Bkv, Lk), K.view3(t["v"], Bkv, Lk), B, Bkv, H, Lq, Lk, self.scale,
                   K.view3(od, B, Lq), lse, drop=spec, **{k_: v_ for k_, v_ in kw.items() if k_ != "biasT"})
        return od, lse

    def backward(self, spec, fwd, phase=0, into=None, ask_form=False):
        K, B, Bkv, H, Lq, Lk = self.K, self.B, self.Bkv, self.H, self.Lq, self.Lk
        kw, t = self._device()
        od, lse = fwd
        nan = lambda x: torch.full_like(x, float("nan"))
        dq, dk, dv, delta = into if into is not None else (nan(t["q"]), nan(t["k"]), nan(t["v"]), nan(lse))
        dS = torch.zeros(B, H, Lq, self.Lkp, device=dev, dtype=torch.bfloat16) if self.bias is not None else None
        form = K.attn_bwd(K.view3(t["q"], B, Lq), K.view3(t["k"], Bkv, Lk), K.view3(t["v"], Bkv, Lk), K.view3(od, B, Lq), K.view3(t["do"], B, Lq),
                          B, Bkv, H, Lq, Lk, self.scale, lse, delta, K.view3(dq, B, Lq), K.view3(dk, Bkv, Lk), K.view3(dv, Bkv, Lk),
                          dS=dS, phase=phase, ask_form=ask_form, drop=spec, **kw)
        return form if ask_form else (dq, dk, dv, delta, dS)

    # ---- metrics ----
    def err(self, got, ref, B_, L_):
        """max of relerr and the per-(sequence, head) slice_relerr(floor=0.05) of a [B_ * L_, H * d] device tensor"""
        H, d = self.H, self.d
        bh = lambda t: t.detach().cpu().double().reshape(B_, L_, H, d).permute(0, 2, 1, 3).reshape(B_ * H, L_ * d)
        return max(relerr(got.view(B_, L_, H * d), ref), slice_relerr(bh(got), bh(ref), floor=0.05))

    def forward_errors(self, ref, fwd):
        od, lse = fwd
        assert bool(torch.isfinite(lse).all())
        return {"out": self.err(od, ref["out"], self.B, self.Lq)}

    def backward_errors(self, ref, bwd):
        dq, dk, dv, delta, dS = bwd
        assert bool(torch.isfinite(delta).all())
        e = {"dq": self.err(dq, ref["dq"], self.B, self.Lq), "dk": self.err(dk, ref["dk"], self.Bkv, self.Lk),
             "dv": self.err(dv, ref["dv"], self.Bkv, self.Lk)}
        if self.bias is not None:
            got = dS[..., :self.Lk].float().sum(0)
            e["dS"] = max(relerr(got, ref["dS"]), slice_relerr(got, ref["dS"], floor=0.05))         # head by head
        return e


def assert_within(errs, label):
    for name, e in errs.items():
        assert e < (TOL_OUT if name == "out" else TOL_GRAD), (label, name, e, errs)


def run_both_forms(case, spec, ref, form, label):
    """forward + backward against `ref`; a case whose default backward is the one-pass grouped kernel (form 2) runs again as the dQ + dK/dV pair
    under x2_tune(14, 1), against the same reference.  Returns {tensor: worst error} and the default run's tensors."""
    fwd = case.forward(spec)
    worst = case.forward_errors(ref, fwd)
    assert_within(worst, label)
    assert case.backward(spec, fwd, ask_form=True) == form, label
    got = case.backward(spec, fwd)
    errs = case.backward_errors(ref, got)
    assert_within(errs, label)
    worst.update(errs)
    if form == 2:
        with tuned({14: 1}):
            assert case.backward(spec, fwd, ask_form=True) == 0, label
            errs = case.backward_errors(ref, case.backward(spec, fwd))
        assert_within(errs, label + " as the pair")
        worst = {n: max(e, errs.get(n, 0.0)) for n, e in worst.items()}
    return worst, fwd, got


def show(label, worst):
    print("dropout attention %-34s %s" % (label, "  ".join("%s %.2e" % kv for kv in worst.items())))


SHARED_197 = dict(B=6, Bkv=3, H=3, Lq=30, Lk=197, use_mask=True, kv_map=[0, 2, 1, 1, 0, 1])
# Every branch of x2_attn_fwd / x2_attn_bwd (csrc/attention.hip) that launches a kernel reading the dropout spec; `form` is what
# x2_attn_bwd_one_pass answers with dropout on (forms 1 and 3 never run then).  Form 2 cases run the pair as well (run_both_forms).
ATTN_CASES = {
    # fwd<2,1,true,1>; dq<2,1,true,1>; dkv<2,1,true,1> (Lk <= 32, one sequence per K/V batch)
    "30x30": dict(B=3, Bkv=3, H=3, Lq=30, Lk=30, use_mask=True, form=0),
    # the same forward / dQ kernels at both upper limits (Lq = 32, Lk = 64); dkv<4,1,false> (Lk > 32)
    "32x64": dict(B=2, Bkv=2, H=2, Lq=32, Lk=64, use_mask=True, form=0),
    # fwd<4,1,false>; dq<4,1,false>; dkv<4,1,false> - a ragged single tile, then a full one
    "40x40": dict(B=2, Bkv=2, H=2, Lq=40, Lk=40, use_mask=True, form=0),
    "64x64": dict(B=2, Bkv=2, H=2, Lq=64, Lk=64, use_mask=True, form=0),
    # fwd<2,1,false> over 4 key tiles; form 2 = onepass_grouped<true>; as the pair: dq_grouped<8> + dkv<4,1,false> over the CSR
    "30x197-shared": dict(SHARED_197, form=2),
    # 9 rows on one image + 2 on another: fwd<2,1,false>; form 2 with three 4-sequence chunks; as the pair: dq_grouped<8> + dkv<4,1,false>
    "30x70-shared-9+2": dict(B=11, Bkv=2, H=3, Lq=30, Lk=70, use_mask=True, kv_map=[0] * 9 + [1] * 2, form=2),
    # fwd<2,1,false> over 10 key tiles; dq<2,1,false> (Lk > 256: neither one pass nor grouped); dkv<4,1,false> over the CSR
    "30x577-shared": dict(B=4, Bkv=2, H=2, Lq=30, Lk=577, use_mask=True, kv_map=[1, 0, 1, 1], form=0),
    # Lk <= 32 with a CSR: fwd<2,1,true,1>; by default this geometry too is form 2 (onepass_grouped<true>, one ragged strip of keys); as the
    # pair: dq_grouped<8> + dkv<2,1,false>
    "30x20-shared": dict(B=4, Bkv=2, H=2, Lq=30, Lk=20, kv_map=[1, 0, 1, 1], form=2),
    # strip-walking resident kernels: fwd_walk<4>; dq_walk<4>; dkv<8,1,true> (resident Q / dO: the LEAN tile with compile-time DROP)
    "70x70-bias": dict(B=2, Bkv=2, H=3, Lq=70, Lk=70, use_bias=True, form=0),
    "100x208-bias": dict(B=2, Bkv=2, H=2, Lq=100, Lk=208, use_bias=True, form=0),
    # ... and their log2-bias instantiations: fwd_walk<4,true>; dq_walk<4,true>; dkv<8,1,true,4,4,true>
    "100x208-bias-log2": dict(B=2, Bkv=2, H=2, Lq=100, Lk=208, use_bias=True, bias_log2=True, form=0),
    # 208 < Lk <= 256: fwd<8,1,true>; dq<8,1,true>; dkv<8,1,true> - bias + mask, two query tiles, two key blocks
    "130x230-bias-mask": dict(B=2, Bkv=2, H=2, Lq=130, Lk=230, use_bias=True, use_mask=True, form=0),
    # kv_idx keeps Lq > 64 off the walk kernel: fwd<8,1,true>; form 2 = onepass_grouped<true> with 70-query sequences; as the pair:
    # dq_grouped<8> + dkv<4,1,false> (a CSR: never the resident kernel)
    "70x100-shared": dict(B=3, Bkv=2, H=2, Lq=70, Lk=100, use_mask=True, kv_map=[0, 1, 1], form=2),
    # 8-wave streamed kernels: fwd<8,1,false>; dq<8,1,false>; dkv<8,1,true> (Lq <= 256) - and the BL2 instantiations of all three
    "130x300-bias": dict(B=2, Bkv=2, H=2, Lq=130, Lk=300, use_bias=True, form=0),
    "130x300-bias-log2": dict(B=2, Bkv=2, H=2, Lq=130, Lk=300, use_bias=True, bias_log2=True, form=0),
    # two ragged 128-query tiles beyond the first; dkv<8,1,false> (Lq > 256: Q / dO streamed)
    "300x300-bias": dict(B=2, Bkv=2, H=3, Lq=300, Lk=300, use_bias=True, form=0),
    # fwd<4,1,false> through Lk > 256 (Lq <= 64); dq<4,1,false>; dkv<8,1,false>
    "64x300": dict(B=2, Bkv=2, H=2, Lq=64, Lk=300, use_mask=True, form=0),
}


def make_case(K, name, seed):
    kw = dict(ATTN_CASES[name])
    kw.pop("form")
    return AttnCase(K, seed=seed, **kw)


@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_attention_dropout_against_float64(K, name):
    case = make_case(K, name, seed=1000 + 10 * list(ATTN_CASES).index(name))
    spec = K.dropout_spec(0.1, 4242, 5)
    worst, _, _ = run_both_forms(case, spec, case.reference_for(spec), ATTN_CASES[name]["form"], name)
    show(name, worst)


@pytest.mark.parametrize("name", ["30x30", "30x197-shared"])
def test_attention_dropout_at_one_half(K, name):
    """p = 0.5: threshold 32768, survivors scaled by 2"""
    case = make_case(K, name, seed=2000)
    spec = K.dropout_spec(0.5, 99, 2)
    assert spec[0] == 32768 and spec[2] == 2.0
    worst, _, _ = run_both_forms(case, spec, case.reference_for(spec), ATTN_CASES[name]["form"], name)
    show(name + " p=0.5", worst)


@pytest.mark.parametrize("name", ["130x230-bias-mask", "30x197-shared"])
def test_attention_dropout_phase_split_gives_the_same_bits(K, name):
    """phase 1 (dQ, dS, delta) then phase 2 (dK / dV from that delta) as separate calls = the dQ + dK/dV pair in one call, bit for bit, with the
    masks regenerated in each: own K/V (form 0 by default) and rows sharing K/V (the pair under x2_tune(14, 1))."""
    case = make_case(K, name, seed=2100)
    spec = K.dropout_spec(0.1, 777, 3)
    with tuned({14: 1}):
        fwd = case.forward(spec)
        assert case.backward(spec, fwd, ask_form=True) == 0
        dq, dk, dv, delta, dS = case.backward(spec, fwd)
        into = tuple(torch.zeros_like(t) for t in (dq, dk, dv, delta))
        _, _, _, _, dS1 = case.backward(spec, fwd, phase=1, into=into)
        assert torch.equal(into[0], dq) and float(into[1].float().abs().max()) == 0.0 and float(into[2].float().abs().max()) == 0.0
        assert dS is None or torch.equal(dS1, dS)
        case.backward(spec, fwd, phase=2, into=into)
        assert torch.equal(into[1], dk) and torch.equal(into[2], dv) and torch.equal(into[3], delta) and torch.equal(into[0], dq)
    assert_within(case.backward_errors(case.reference_for(spec), (dq, dk, dv, delta, dS)), name)


def test_attention_dropout_follows_the_device_epoch(K):
    """An int32 [1] device tensor in the spec's fourth slot (what a replayed hipGraph step hands over): every kernel of the site mixes it into the
    seed.  Epochs 5, 6, 5: each run matches the float64 reference mirrored at that epoch, runs 1 and 3 are the same bits, runs 1 and 2 differ."""
    case = make_case(K, "30x197-shared", seed=2200)
    epoch = torch.tensor([5], dtype=torch.int32, device=dev)
    spec = K.dropout_spec(0.1, 31337, 4)[:3] + (epoch,)
    refs, runs, worst = {}, [], {}
    for e in (5, 6, 5):
        epoch.fill_(e)
        if e not in refs:
            refs[e] = case.reference_for(spec)
        w, fwd, bwd = run_both_forms(case, spec, refs[e], 2, "epoch %d" % e)
        worst = {n: max(v, worst.get(n, 0.0)) for n, v in w.items()}
        runs.append([fwd[0]] + list(bwd[:3]))
    assert not torch.equal(refs[5]["out"], refs[6]["out"])
    for a_, b_ in zip(runs[0], runs[2]):
        assert torch.equal(a_, b_)
    for a_, b_ in zip(runs[0], runs[1]):
        assert not torch.equal(a_, b_)
    show("30x197-shared epochs 5, 6, 5", worst)


@pytest.mark.parametrize("name", ["30x30", "30x197-shared", "130x300-bias"])
def test_attention_dropout_gate_has_teeth(K, name):
    """The comparison above would see a mask that is off by one key or built with row pitch Lk: the device result is further than 10 x the
    tolerance from references mutated that way (the true and the mutated references differ by 0.58 - 1.09 of max-abs, checked on the CPU)."""
    case = make_case(K, name, seed=2300)
    spec = K.dropout_spec(0.1, 2024, 6)
    assert case.Lk != case.Lkp
    fwd = case.forward(spec)
    dv = case.backward(spec, fwd)[2]
    shown = {}
    for kind, index_kw in (("shifted", dict(shift=1)), ("pitch", dict(pitch=case.Lk))):
        bad = case.reference_for(spec, **index_kw)
        e_out = relerr(fwd[0].view(case.B, case.Lq, -1), bad["out"])
        e_dv = relerr(dv.view(case.Bkv, case.Lk, -1), bad["dv"])
        shown.update({kind + " out": e_out, kind + " dv": e_dv})
        assert e_out > 10 * TOL_OUT and e_dv > 10 * TOL_GRAD, (name, kind, e_out, e_dv)
    show(name + " vs mutated refs", shown)


# ------------------------------------------------------------------------------------------------ NT GEMM epilogue

# (161, 264, 64): one row past a 160-row tile, 8 columns past a 256-column tile
GEMM_SHAPES = [(300, 200, 192), (161, 264, 64), (97, 136, 128)]
_GEMM = {}


def gemm_case(M, N, K_):
    """operands (bf16-rounded), epilogue inputs and the float64 product of one shape - built once, shared, never written to"""
    if (M, N, K_) not in _GEMM:
        A, B = bf(rnd(M, K_, seed=61)), bf(rnd(N, K_, seed=62, scale=K_ ** -0.5))
        c = dict(A=A, B=B, ref=A.double() @ B.double().t(), bias=rnd(N, seed=63), gamma=rnd(N, seed=64), resid=rnd(M, N, seed=65),
                 rowscale=(torch.rand(M, generator=torch.Generator().manual_seed(66)) > 0.2).float() * 1.25,
                 idx=torch.arange(M).unsqueeze(1) * N + torch.arange(N).unsqueeze(0))
        c["pre"] = c["ref"] + c["bias"].double()
        # no product is so small that adding it to the residual could leave the residual's bits unchanged
        assert bool((c["pre"].abs() > 1e-6 * c["resid"].abs().clamp_min(1.0).double()).all())
        c["dev"] = {n: c[n].to(dev) for n in ("A", "B", "bias", "gamma", "resid", "rowscale")}
        _GEMM[(M, N, K_)] = c
    return _GEMM[(M, N, K_)]


def same_bits(a, b):
    return a.contiguous().view(torch.int32) == b.contiguous().view(torch.int32)


def check_variant5(out, c, keep):
    """out = resid + keep * (A B^T + bias) to the fp32-out tolerance, and the exact mask: the residual's own bits wherever the mirror drops,
    something else wherever it keeps"""
    out = out.cpu()
    assert rowerr(out, c["resid"].double() + keep * c["pre"]) < 1e-5
    dropped = keep == 0
    assert bool(dropped.any()) and bool(same_bits(out, c["resid"])[dropped].all())
    assert bool((out != c["resid"])[~dropped].all())


@pytest.mark.parametrize("M,N,K_", GEMM_SHAPES)
def test_gemm_nt_bias_dropout_residual(K, M, N, K_, nt_tile):
    """epilogue variant 5 (bias + dropout + residual -> fp32, nt_epilogue_f4): the hidden-dropout launch of the text and fusion layers"""
    c = gemm_case(M, N, K_)
    d = c["dev"]
    spec = K.dropout_spec(0.1, 4321, 3)
    out = K.gemm_nt(d["A"], d["B"], bias=d["bias"], resid=d["resid"], out_dtype=torch.float32, drop=spec)
    check_variant5(out, c, K.dropout_keep(spec, c["idx"]).double())


@pytest.mark.parametrize("M,N,K_", GEMM_SHAPES)
def test_gemm_nt_dropout_follows_the_device_epoch(K, M, N, K_, nt_tile):
    c = gemm_case(M, N, K_)
    d = c["dev"]
    epoch = torch.tensor([5], dtype=torch.int32, device=dev)
    spec = K.dropout_spec(0.1, 4321, 3)[:3] + (epoch,)
    outs = []
    for e in (5, 6, 5):
        epoch.fill_(e)
        out = K.gemm_nt(d["A"], d["B"], bias=d["bias"], resid=d["resid"], out_dtype=torch.float32, drop=spec)
        check_variant5(out, c, K.dropout_keep(spec, c["idx"]).double())
        outs.append(out)
    assert torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("M,N,K_", GEMM_SHAPES)
def test_gemm_nt_dropout_into_a_column_slice(K, M, N, K_, nt_tile):
    """ldc > N: the mask is still a function of m * N + n (the problem's N, not the output's row pitch), nothing is written outside the slice"""
    c = gemm_case(M, N, K_)
    d = c["dev"]
    spec = K.dropout_spec(0.1, 4321, 3)
    wide = torch.zeros(M, N + 64, device=dev)
    K.gemm_nt(d["A"], d["B"], bias=d["bias"], resid=d["resid"], out=wide[:, 32:32 + N], drop=spec)
    check_variant5(wide[:, 32:32 + N], c, K.dropout_keep(spec, c["idx"]).double())
    assert float(wide[:, :32].abs().max()) == 0.0 and float(wide[:, 32 + N:].abs().max()) == 0.0
    assert torch.equal(wide[:, 32:32 + N], K.gemm_nt(d["A"], d["B"], bias=d["bias"], resid=d["resid"], out_dtype=torch.float32, drop=spec))


@pytest.mark.parametrize("M,N,K_", GEMM_SHAPES)
def test_gemm_nt_layerscale_with_droppath_rows(K, M, N, K_, nt_tile):
    """epilogue variant 6 with DropPath row factors (0 or 1.25): resid + rowscale[m] * gamma * (A B^T + bias)"""
    c = gemm_case(M, N, K_)
    d = c["dev"]
    out = K.gemm_nt(d["A"], d["B"], bias=d["bias"], gamma=d["gamma"], resid=d["resid"], out_dtype=torch.float32, rowscale=d["rowscale"]).cpu()
    rs = c["rowscale"].double().unsqueeze(1)
    assert rowerr(out, c["resid"].double() + rs * c["gamma"].double() * c["pre"]) < 1e-5
    dead = c["rowscale"] == 0
    assert 0 < int(dead.sum()) < M and bool(same_bits(out, c["resid"])[dead].all())


@pytest.mark.parametrize("M,N,K_", GEMM_SHAPES)
def test_gemm_nt_generic_epilogue_with_dropout(K, M, N, K_, nt_tile128):
    """bias + gamma + dropout -> bf16 is none of the compiled feature sets: the generic epilogue (variant 4).  The 256-column and ping-pong kernels
    refuse variant 4 - such a launch falls to the 128-column family whatever knobs 1 and 15 say - so this runs under the four tile* ids only."""
    c = gemm_case(M, N, K_)
    d = c["dev"]
    spec = K.dropout_spec(0.1, 4321, 3)
    keep = K.dropout_keep(spec, c["idx"]).double()
    out = K.gemm_nt(d["A"], d["B"], bias=d["bias"], gamma=d["gamma"], drop=spec).cpu()
    assert out.dtype == torch.bfloat16 and rowerr(out, c["gamma"].double() * keep * c["pre"]) < 6e-3
    assert bool((out[keep == 0] == 0).all()) and bool((out[keep != 0] != 0).all())


def test_nt_tile_fixture_sets_the_knobs(nt_tile):
    """a silently ignored knob would turn the twelve variants above into one"""
    lib = _lib()
    assert (lib.x2_tune_get(1), lib.x2_tune_get(3), lib.x2_tune_get(15)) == tuple(nt_tile)
