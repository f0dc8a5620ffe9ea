"""Where the kernels write: every entry point below runs through the C ABI on outputs and workspaces of exactly the size include/x2vlm_hip.h
documents, each inside one flat allocation whose every other byte holds a sentinel bit pattern (`guarded`).  A case asserts the values against
float64 at the tolerance the older kernel tests use (1e-5 of max-abs for fp32 outputs, 6e-3 for bf16 outputs, 1.5e-2 for the attention backward,
bit-exact where they are) AND that every guard, row gap and batch gap still holds the pattern.  Inputs are slices of NaN-filled buffers: a read
outside the documented extent turns a result NaN.  Guards are sized for the largest tile (256 rows x ld behind a 2-D output, one more unit of the
layout behind a workspace, 4096 elements in front), so an overrun is a failed assertion inside the allocation, not a fault.

Entry point -> extent held here (header sentence):
  x2_gemm_nt                 C [M][ldc], aux [M][ldaux], colsum [N]                      twelve tile families + automatic
  x2_gemm_nt_dgelu_colparts  C [M][ldc], colparts 2 * ceil(M / 64) * N, *nrows_out <= 2 * ceil(M / 64)
  x2_gemm_nt_splitk          C [M][ldc], ws slices * M * N; "clamped to ws_floats / (M*N)"; ws = NULL
  x2_gemm_tn_grouped         dW [N][ld_dW], ws split * tiles256 * 65536; explicit split, split = 0 with room for one slice, a group of three
  x2_attn_fwd / x2_attn_bwd  Out, dQ, dK, dV strided per row and per sequence; LSE, Delta [B][H][Lq]; dS [B][H][Lq][ds_ld]; colsum_ws [B][2][H*64];
                             ws B * H * ceil(Lq / 128) * 8192 (one float fewer: x2_attn_bwd_one_pass == 0, the pair runs); x2_tune(14, 1); phases 1 / 2
  x2_attn_fwd_mask2d / x2_attn_bwd_mask2d   the same outputs
  x2_layernorm_fwd           y_bf16 / y_f32 [rows(+cls)][D], mean / rstd [rows]; x2_tune(13, v)
  x2_layernorm_bwd           dx, dx_bf16, dw / db / dcol [D], ws ceil(rows / 16) * 3 * D; defer 0 / 1
  x2_colsum_bf16             out [N], ws ceil(M / 64) * N
  x2_rowscale_cast_colsum    dx_bf16 [M][D], colsum [D], ws ceil(M / 32) * D
  x2_reduce_partials(_multi) outputs [width], a null output slot
  x2_layerscale_finish       G [N][K], dgamma / dbias [N]
  x2_cast_transpose_bf16 / _multi   dst [R][C], dstT [C][ldt]
  x2_relpos_bias / _bwd      bias / biasT [H][N][ld] with zero pad columns; dtable [T][H], ws slices * H * N * ld
  x2_mlm_ce_fwd / x2_ce_combine / x2_mlm_ce_bwd and x2_mlm_ls_fwd / x2_ls_combine / x2_mlm_ls_bwd
                             part [R][Vp/64][2], sumz [R][Vp/64], zlab / zign / lse / loss_row [R], out2 [2], dl [R][ldd]
  x2_embed_bwd / _bwd_pid    dword [V][D], dpos [P][D], dtype0 = row 0 of [2][D], scratch min(L, R) * D
  x2_kv_csr, x2_tail_index, x2_additive_mask(2d), x2_mask_tokens, x2_droppath_rows, x2_frame_mean, x2_sample_negatives   every output
and the wrappers of kernels.py that ask kernels.workspace() for scratch, with workspace() handing out guarded buffers of exactly the size asked for
(inline and under kernels.DEFERRED).

LSE bound (test_attention_extents): LSE = log2(e) * logsumexp(scale * q.k + bias + mask).  A float32 torch restatement of that formula differs
from float64 by at most 1.21e-6 on this file's inputs (measured on the CPU: the worst of all geometries below, at Lq = 641, Lk = 769 where |LSE| reaches
11.6; each case prints its own figure); the device bound is 8 times that, LSE_BOUND = 9.68e-6 absolute (the margin covers the device's exp2 / log2
approximations and the MFMA summation order).  Delta = rowsum(dO * O) over a head's 64 columns of the bf16 O the kernel wrote: 1e-5 of max-abs."""
import ctypes as C
import importlib
import math

import pytest
import torch

from kernel_helpers import (BF16, F32, I32, I64, NT_IDS, NT_TILES, SENTINEL, _ALIVE, _INT_OF, K, bf, filled, guarded, lib,  # noqa: F401 (fixtures)
                            nt_pinned, relerr, rnd, tn_tile, tuned)

pytestmark = pytest.mark.gpu
dev = "cuda"

# ------------------------------------------------------------------------------------------------ fixtures, references

@pytest.fixture(autouse=True)
def _release_allocations():
    yield
    if _ALIVE and _ALIVE[0].is_cuda:
        torch.cuda.synchronize()
    del _ALIVE[:]


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def dgelu64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def ceil_div(a, b):
    return (a + b - 1) // b


def all_ok(*guards):
    torch.cuda.synchronize()
    for g in guards:
        g()


# ------------------------------------------------------------------------------------------------ 1. the helper has teeth on the device

def test_guard_reports_a_workspace_one_partial_row_short(K):
    """x2_colsum_bf16 writes ceil(M / 64) partial rows of N floats.  Declared one partial row short, the second row lands in the trailing guard (inside
    the allocation) and the checker names it; with the documented size the same call leaves every guard intact."""
    M, N = 65, 8
    y = filled(bf(rnd(M, N, seed=1)), ld=N + 8)
    for rows_declared, want in ((1, ("tail", 1, 0)), (2, None)):
        ws, g_ws = guarded((rows_declared * N,), F32, tail=N, name="ws")
        out, g_out = guarded((N,), F32, name="out")
        out.zero_()
        K.call("x2_colsum_bf16", K.ptr(y), K.ptr(out), M, N, N + 8, K.ptr(ws), 0)
        torch.cuda.synchronize()
        g_out()
        assert g_ws.bad() == want, g_ws.bad()
        if want is not None:
            with pytest.raises(AssertionError, match="ws: write outside the extent: region tail, row 1, column 0"):
                g_ws()


# ------------------------------------------------------------------------------------------------ 2. GEMMs

@pytest.fixture(params=[(0, 0, 0)] + NT_TILES, ids=["auto"] + NT_IDS)
def nt_tile(request):
    with nt_pinned(request.param):
        yield request.param


_NT_REF = {}


def nt_operands(M, N, Kd):
    """operands as column slices of wider NaN-filled buffers + the float64 product, computed once per shape"""
    key = (M, N, Kd)
    if key not in _NT_REF:
        A, B = bf(rnd(M, Kd, seed=M + 1)), bf(rnd(N, Kd, seed=N + 2, scale=Kd ** -0.5))
        bias, resid, pre = rnd(N, seed=3), rnd(M, N, seed=5), bf(rnd(M, N, seed=6))
        _NT_REF[key] = (A, B, bias, resid, pre, A.double() @ B.double().t())
    A, B, bias, resid, pre, ref = _NT_REF[key]
    return filled(A, ld=Kd + 16), filled(B, ld=Kd + 8), filled(bias), filled(resid, ld=N + 4), filled(pre, ld=N + 8), bias, resid, pre, ref


@pytest.mark.parametrize("M,N,Kd", [(1, 8, 64), (33, 72, 64), (257, 264, 128)])
def test_gemm_nt_extents(K, nt_tile, M, N, Kd):
    Ad, Bd, biasd, residd, pred, bias, resid, pre, ref = nt_operands(M, N, Kd)
    ldc = N + 8

    def run(out_f32, act=0, bias_=None, resid_=None, aux=None, colsum=None):
        Cv, gC = guarded((M, N), F32 if out_f32 else BF16, ld=ldc, name="C")
        K.call("x2_gemm_nt", K.ptr(Ad), K.ptr(Bd), K.ptr(Cv), M, N, Kd, Kd + 16, Kd + 8, ldc, K.ptr(bias_), None, K.ptr(resid_), N + 4 if resid_ is not None else 0,
               K.ptr(aux), N + 8 if aux is not None else 0, act, 1 if out_f32 else 0, 0, 0, 1.0, None, None, K.ptr(colsum))
        return Cv, gC

    for out_f32 in (True, False):
        tol = 1e-5 if out_f32 else 6e-3
        Cv, gC = run(out_f32)
        all_ok(gC)
        assert relerr(Cv, ref) < tol
        # bias + GELU with the pre-activation saved at ldaux = N + 8
        aux, gA = guarded((M, N), BF16, ld=N + 8, name="aux")
        Cv, gC = run(out_f32, act=1, bias_=biasd, aux=aux)
        all_ok(gC, gA)
        assert relerr(Cv, gelu64(ref + bias.double())) < tol and relerr(aux, ref + bias.double()) < 6e-3
        # bias + residual at ldr = N + 4
        Cv, gC = run(out_f32, bias_=biasd, resid_=residd)
        all_ok(gC)
        assert relerr(Cv, ref + bias.double() + resid.double()) < tol
        # GELU' of a saved pre-activation + the fused column sums into a guarded [N] vector
        cs, gS = guarded((N,), F32, name="colsum")
        cs.fill_(2.0)
        Cv, gC = run(out_f32, act=2, aux=pred, colsum=cs)
        all_ok(gC, gS)
        want = ref * dgelu64(pre.double())
        assert relerr(Cv, want) < tol and relerr(cs - 2.0, want.sum(0)) < 2e-5


@pytest.mark.parametrize("tile", [0, 1, 2, 3], ids=["auto", "tile128", "tile192", "tile64"])
@pytest.mark.parametrize("M,N,Kd", [(1, 8, 64), (65, 72, 64), (130, 64, 64), (193, 136, 128)])
def test_gemm_nt_dgelu_colparts_extents(K, lib, M, N, Kd, tile):
    Ad, Bd, _, _, pred, _, _, pre, ref = nt_operands(M, N, Kd)
    rows = 2 * ceil_div(M, 64)
    with tuned({1: 1, 3: tile}):
        Cv, gC = guarded((M, N), BF16, ld=N + 8, name="C")
        parts, gP = guarded((rows * N,), F32, tail=2 * N, name="colparts")
        nrows = C.c_int(-1)
        K.call("x2_gemm_nt_dgelu_colparts", K.ptr(Ad), K.ptr(Bd), K.ptr(Cv), M, N, Kd, Kd + 16, Kd + 8, N + 8, K.ptr(pred), N + 8, K.ptr(parts), C.byref(nrows))
        all_ok(gC, gP)
        assert 1 <= nrows.value <= rows
        want = ref * dgelu64(pre.double())
        assert relerr(Cv, want) < 6e-3
        cs, gS = guarded((N,), F32, name="colsum")
        cs.fill_(3.0)
        K.call("x2_reduce_partials", K.ptr(parts), nrows.value, 1, N, K.ptr(cs), None, None)
        all_ok(gS, gP)
        # the partial rows sum the fp32 values before their bf16 rounding: the project's fp32 bound against the column's absolute sum
        assert float((cs.cpu().double() - 3.0 - want.sum(0)).abs().max()) <= 1e-5 * float(want.abs().sum(0).max()) + 1e-6


def test_gemm_nt_splitk_extents(K):
    """exact 3 * M * N floats for three slices; ten slices and automatic with room for two ("clamped to ws_floats / (M*N)"); no workspace; strided C"""
    for (M, N, Kd, slices, room) in ((33, 72, 1024, 3, 3), (130, 136, 640, 10, 2), (130, 136, 640, 0, 2), (130, 136, 640, 10, 0), (33, 72, 1024, 3, 1)):
        A, B = bf(rnd(M, Kd, seed=11)), bf(rnd(N, Kd, seed=12, scale=Kd ** -0.5))
        ref = A.double() @ B.double().t()
        Ad, Bd = filled(A, ld=Kd + 8), filled(B, ld=Kd + 16)
        Cv, gC = guarded((M, N), F32, ld=N + 12, name="C")
        ws, gW = guarded((max(room, 1) * M * N,), F32, tail=M * N, name="ws")
        K.call("x2_gemm_nt_splitk", K.ptr(Ad), K.ptr(Bd), K.ptr(Cv), M, N, Kd, Kd + 8, Kd + 16, N + 12, slices, K.ptr(ws) if room else None, room * M * N)
        all_ok(gC, gW)
        assert relerr(Cv, ref) < 1e-5, (M, N, Kd, slices, room)
        if room <= 1:      # nothing passes through a workspace that holds fewer than two slices
            assert bool((ws.view(I32) == SENTINEL[F32]).all())


def tn_problem(Mc, N, Kd, seed):
    dY, X = bf(rnd(Mc, N, seed=seed)), bf(rnd(Mc, Kd, seed=seed + 1))
    n_ld = ceil_div(N, 8) * 8
    return filled(dY, ld=n_ld + 8), filled(X, ld=Kd + 8), n_ld, dY.double().t() @ X.double()


def tn_call(K, probs, accumulate, split, ws, ws_floats):
    """probs: (dY view, X view, dW view, N, K, n_ld)"""
    flat = []
    for dY, X, dW, N, Kd, n_ld in probs:
        flat += [dY.data_ptr(), X.data_ptr(), dW.data_ptr(), dY.shape[0], N, Kd, dY.stride(0), X.stride(0), dW.stride(0), n_ld, Kd]
    K.call("x2_gemm_tn_grouped", (C.c_int64 * len(flat))(*flat), len(probs), accumulate, split, K.ptr(ws) if ws is not None else None, ws_floats)


@pytest.mark.parametrize("Mc,N,Kd", [(64, 8, 8), (100, 136, 72), (192, 264, 320), (33, 256, 256)])
def test_gemm_tn_grouped_extents(K, tn_tile, Mc, N, Kd):
    dY, X, n_ld, ref = tn_problem(Mc, N, Kd, seed=Mc)
    tiles256 = ceil_div(N, 256) * ceil_div(Kd, 256)
    # (split, slices of room in the workspace): no workspace; split = 0 with room for one slice; explicit splits with exactly their size (256x256 kernel)
    plans = [(0, 0), (1, 0), (0, 1)] + ([(2, 2), (3, 3)] if tn_tile == 2 else [])
    for split, room in plans:
        for accumulate in (0, 1):
            dW, gW = guarded((N, Kd), F32, ld=Kd + 4, name="dW")
            dW.fill_(1.5)
            ws, gS = guarded((max(room, 1) * tiles256 * 65536,), F32, tail=65536, name="ws")
            tn_call(K, [(dY, X, dW, N, Kd, n_ld)], accumulate, split, ws if room else None, room * tiles256 * 65536)
            all_ok(gW, gS)
            assert relerr(dW, ref + (1.5 if accumulate else 0.0)) < 1e-5, (split, room, accumulate)
            if room <= 1:
                assert bool((ws.view(I32) == SENTINEL[F32]).all())


def test_gemm_tn_group_back_to_back(K, tn_tile):
    """three problems whose dW sit back to back in ONE guarded buffer (an overrun of one lands in the guard or visibly in the next), padded n_ld"""
    shapes = [(100, 136, 72), (64, 8, 8), (33, 250, 64)]
    total = sum(N * Kd for _, N, Kd in shapes)
    buf, gB = guarded((total,), F32, tail=65536, name="dW x 3")
    tiles256 = sum(ceil_div(N, 256) * ceil_div(Kd, 256) for _, N, Kd in shapes)
    for split, room in ((0, 0), (0, 1)) + (((2, 2),) if tn_tile == 2 else ()):
        buf.fill_(-4.0)
        ws, gS = guarded((max(room, 1) * tiles256 * 65536,), F32, tail=65536, name="ws")
        probs, refs, o = [], [], 0
        for i, (Mc, N, Kd) in enumerate(shapes):
            dY, X, n_ld, ref = tn_problem(Mc, N, Kd, seed=70 + i)
            probs.append((dY, X, buf[o:o + N * Kd].view(N, Kd), N, Kd, n_ld)); refs.append(ref); o += N * Kd
        tn_call(K, probs, 0, split, ws if room else None, room * tiles256 * 65536)
        all_ok(gB, gS)
        for p, r in zip(probs, refs):
            assert relerr(p[2], r) < 1e-5, (split, p[3], p[4])


# ------------------------------------------------------------------------------------------------ 2. attention

LOG2E = 1.4426950408889634
LSE_F32_ERR = 1.21e-6          # worst |float32 restatement - float64| of LSE over this file's inputs, measured on the CPU (see the module docstring)
LSE_BOUND = 8 * LSE_F32_ERR
_ATTN = {}


def heads(t, H):
    """[B, L, H * 64] -> float64 [B, H, L, 64]"""
    B, L, _ = t.shape
    return t.double().view(B, L, H, 64).permute(0, 2, 1, 3)


def unheads(t):
    B, H, L, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, L, H * d)


def attn_case(B, Bkv, H, Lq, Lk, use_bias, use_mask, kv_map, seed, mask2d=False):
    """seeded bf16 inputs and the float64 reference (outputs, LSE, gradients for the dO of the case), computed once per geometry"""
    key = (B, Bkv, H, Lq, Lk, use_bias, use_mask, None if kv_map is None else tuple(kv_map), seed, mask2d)
    if key in _ATTN:
        return _ATTN[key]
    d, scale = 64, 0.125
    q, do = bf(rnd(B, Lq, H * d, seed=seed)), bf(rnd(B, Lq, H * d, seed=seed + 3))
    k, v = bf(rnd(Bkv, Lk, H * d, seed=seed + 1)), bf(rnd(Bkv, Lk, H * d, seed=seed + 2))
    bias = rnd(H, Lq, Lk, seed=seed + 4) if use_bias else None
    mask = None
    g = torch.Generator().manual_seed(seed + 5)
    if use_mask:
        keep = (torch.rand(B, Lk, generator=g) > 0.3).float()
        keep[:, 0] = 1
        mask = (1 - keep) * -10000.0
    m2 = None
    if mask2d:                    # causal x key padding, as the captioning fine-tune builds it
        lens = torch.randint(1, Lq + 1, (B,), generator=g)
        lens[0] = Lq
        allow = torch.tril(torch.ones(Lq, Lk))[None] * (torch.arange(Lk)[None, None, :] < lens[:, None, None]).float()
        m2 = (1 - allow) * -10000.0
    idx = torch.arange(B) if kv_map is None else torch.tensor(kv_map)
    add = torch.zeros(B, H, Lq, Lk, dtype=torch.float64)
    if use_bias:
        add = add + bias.double()[None]
    if use_mask:
        add = add + mask.double()[:, None, None, :]
    if mask2d:
        add = add + m2.double()[:, None]
    q4, do4, k4, v4 = heads(q, H), heads(do, H), heads(k, H)[idx], heads(v, H)[idx]
    S = scale * q4 @ k4.transpose(2, 3) + add
    lse = torch.logsumexp(S, -1)
    P = torch.exp(S - lse[..., None])
    O4 = P @ v4
    dP = do4 @ v4.transpose(2, 3)
    dS = P * (dP - (do4 * O4).sum(-1, keepdim=True))
    dq4 = scale * dS @ k4
    dk4 = torch.zeros(Bkv, H, Lk, d, dtype=torch.float64).index_add_(0, idx, scale * dS.transpose(2, 3) @ q4)
    dv4 = torch.zeros(Bkv, H, Lk, d, dtype=torch.float64).index_add_(0, idx, P.transpose(2, 3) @ do4)
    # the float32 restatement of the header's LSE formula, for the bound on the device's LSE
    S32 = scale * (q4.float() @ k4.float().transpose(2, 3)) + add.float()
    lse32_err = float(((torch.tensor(LOG2E) * torch.logsumexp(S32, -1)).double() - LOG2E * lse).abs().max())
    ref = dict(q=q, k=k, v=v, do=do, bias=bias, mask=mask, m2=m2, idx=idx, scale=scale, out=unheads(O4), lse=(LOG2E * lse).reshape(-1), dq=unheads(dq4),
               dk=unheads(dk4), dv=unheads(dv4), dbias=dS.sum(0), lse32_err=lse32_err)
    _ATTN[key] = ref
    return ref


def attn_struct(mod, B, Bkv, H, Lq, Lk, scale, **t):
    a = mod.AttnArgs()
    a.B, a.Bkv, a.H, a.Lq, a.Lk, a.scale, a.head_dim = B, Bkv, H, Lq, Lk, scale, 64
    for name, pre in (("Q", "q"), ("K", "k"), ("V", "v"), ("dO", "do"), ("dQ", "dq"), ("dK", "dk"), ("dV", "dv"), ("O", "o"), ("Out", "o")):
        x = t.get(name)
        if x is not None:
            setattr(a, name, x.data_ptr()); setattr(a, pre + "_bs", x.stride(0)); setattr(a, pre + "_rs", x.stride(1))
    for name in ("LSE", "Delta", "dS", "bias", "biasT", "mask", "kv_idx", "seq_off", "seq_ids", "ws", "colsum_ws"):
        if t.get(name) is not None:
            setattr(a, name, t[name].data_ptr())
    for name in ("bias_ld", "biasT_ld", "mask_ld", "ds_ld", "ws_floats", "phase"):
        if name in t:
            setattr(a, name, t[name])
    return a


def expected_form(Lq, Lk, shared, has_bias):
    if Lk <= 208:
        if not shared and 64 < Lq <= 208 and Lk > 64:
            return 1
        return 2 if shared and Lq <= 128 and not has_bias else 0
    return 3 if not shared and 208 < Lq <= 640 and Lk <= 768 else 0


def seq3(t, H, L, **kw):
    """a [B, L, H * 64] bf16 host tensor in the strided layout of this file: rows H * 64 + 64 apart, sequences L + 8 rows apart, NaN around"""
    return filled(t, ld=H * 64 + 64, batch_stride=L + 8, **kw)


def out3(B, L, H, name):
    return guarded((B, L, H * 64), BF16, ld=H * 64 + 64, batch_stride=L + 8, name=name)


def run_attention_extents(K, lib, B, Bkv, H, Lq, Lk, use_bias=False, use_mask=False, kv_map=None, seed=0, short_ws=False):
    r = attn_case(B, Bkv, H, Lq, Lk, use_bias, use_mask, kv_map, seed)
    scale, shared = r["scale"], kv_map is not None
    Lkp, Lqp = K.round_up(Lk, 64), K.round_up(Lq, 128 if Lq > 208 else 64)
    qd, kd, vd, dod = seq3(r["q"], H, Lq), seq3(r["k"], H, Lk), seq3(r["v"], H, Lk), seq3(r["do"], H, Lq)
    kw = {}
    if use_bias:          # pad columns hold the zeros x2_relpos_bias writes there
        bp = torch.zeros(H * Lq, Lkp); bp[:, :Lk] = r["bias"].reshape(H * Lq, Lk)
        bT = torch.zeros(H * Lk, Lqp); bT[:, :Lq] = r["bias"].transpose(1, 2).reshape(H * Lk, Lq)
        kw.update(bias=filled(bp), bias_ld=Lkp, biasT=filled(bT), biasT_ld=Lqp)
    if use_mask:          # pad columns hold the zeros x2_additive_mask writes there
        mp = torch.zeros(B, Lkp); mp[:, :Lk] = r["mask"]
        kw.update(mask=filled(mp), mask_ld=Lkp)
    fwd_kws = [dict(kw)]
    if shared:
        kv_idx = torch.tensor(kv_map, dtype=I32)
        off = torch.zeros(Bkv + 1, dtype=I32); off[1:] = torch.cumsum(torch.bincount(kv_idx, minlength=Bkv), 0)
        kw.update(kv_idx=filled(kv_idx), seq_off=filled(off), seq_ids=filled(torch.argsort(kv_idx, stable=True).to(I32)))
        fwd_kws = [{k_: v_ for k_, v_ in kw.items() if k_ not in ("seq_off", "seq_ids")}, dict(kw)]       # per-row kernels, then the grouped one
    for fkw in fwd_kws:
        od, gO = out3(B, Lq, H, "Out")
        lse, gL = guarded((B * H * Lq,), F32, tail=H * Lq, name="LSE")
        a = attn_struct(K, B, Bkv, H, Lq, Lk, scale, Q=qd, K=kd, V=vd, Out=od, LSE=lse, **{k_: v_ for k_, v_ in fkw.items() if k_ != "biasT" and k_ != "biasT_ld"})
        K.call("x2_attn_fwd", C.byref(a))
        all_ok(gO, gL)
        e_out, e_lse = relerr(od, r["out"]), float((lse.cpu().double() - r["lse"]).abs().max())
        print("attention %s fwd: out %.2e lse %.2e (bound %.2e; float32 restatement on the CPU %.2e)" % ((B, Bkv, H, Lq, Lk), e_out, e_lse, LSE_BOUND, r["lse32_err"]))
        assert e_out < 6e-3 and max(relerr(od[b], r["out"][b]) for b in range(B)) < 6e-3
        assert e_lse <= LSE_BOUND
    tol = 1.5e-2
    chunks = ceil_div(Lq, 128)
    ws_floats = B * H * chunks * 8192 - (1 if short_ws else 0)
    want_form = 0 if (short_ws or lib.x2_tune_get(14) == 1) else expected_form(Lq, Lk, shared, use_bias)

    def backward(phase=0, into=None):
        if into is None:
            (dq, gq), (dk, gk), (dv, gv) = out3(B, Lq, H, "dQ"), out3(Bkv, Lk, H, "dK"), out3(Bkv, Lk, H, "dV")
            delta, gD = guarded((B * H * Lq,), F32, tail=H * Lq, name="Delta")
            dS, gS = guarded((B * H * Lq, Lkp), BF16, name="dS") if use_bias else (None, None)
            if dS is not None:
                dS.zero_()
            into = (dq, dk, dv, delta, dS, [g_ for g_ in (gq, gk, gv, gD, gS) if g_ is not None])
        dq, dk, dv, delta, dS, guards = into
        extra = {}
        if Lq > 208 and Lk > 208 and not shared:
            ws, gW = guarded((ws_floats,), F32, tail=8192 + 1, name="ws")
            extra.update(ws=ws, ws_floats=ws_floats)
            guards = guards + [gW]
        a = attn_struct(K, B, Bkv, H, Lq, Lk, scale, Q=qd, K=kd, V=vd, O=od, dO=dod, dQ=dq, dK=dk, dV=dv, LSE=lse, Delta=delta, dS=dS, ds_ld=Lkp,
                        phase=phase, **kw, **extra)
        form = lib.x2_attn_bwd_one_pass(C.byref(a))
        cs = gC = None
        if phase == 0 and form in (1, 3):
            cs, gC = guarded((B * 2 * H * 64,), F32, tail=2 * H * 64, name="colsum_ws")
            a.colsum_ws = cs.data_ptr()
            guards = guards + [gC]
        K.call("x2_attn_bwd", C.byref(a))
        all_ok(*guards)
        return dq, dk, dv, delta, dS, guards, form, cs

    def check(dq, dk, dv, delta, dS, guards, form, cs):
        errs = relerr(dq, r["dq"]), relerr(dk, r["dk"]), relerr(dv, r["dv"])
        want_delta = (dod.float().cpu().double() * od.float().cpu().double()).reshape(B, Lq, H, 64).sum(-1).permute(0, 2, 1).reshape(-1)
        e_delta = relerr(delta, want_delta)
        print("attention %s bwd form %d: dq %.2e dk %.2e dv %.2e delta %.2e" % ((B, Bkv, H, Lq, Lk), form, *errs, e_delta))
        assert max(errs) < tol and e_delta < 1e-5
        for b in range(B):
            assert relerr(dq[b], r["dq"][b]) < tol
        if use_bias:
            dSh = dS.view(B, H, Lq, Lkp).float().cpu()
            assert relerr(dSh[..., :Lk].sum(0), r["dbias"]) < tol
            assert Lkp == Lk or float(dSh[..., Lk:].abs().max()) == 0.0          # the pad columns keep the caller's zeros
        if cs is not None:
            c = cs.view(B, 2, H * 64)
            assert relerr(c[:, 0], dq.float().cpu().sum(1)) < 2e-6 and relerr(c[:, 1], dv.float().cpu().sum(1)) < 2e-6

    got = backward()
    assert got[6] == want_form, (got[6], want_form)
    check(*got)
    if got[6] == 0:
        # the two halves as separate calls on fresh guarded buffers: phase 1 leaves dK / dV untouched (still the sentinel), phase 2 leaves dQ alone
        (dq, gq), (dk, gk), (dv, gv) = out3(B, Lq, H, "dQ"), out3(Bkv, Lk, H, "dK"), out3(Bkv, Lk, H, "dV")
        delta, gD = guarded((B * H * Lq,), F32, tail=H * Lq, name="Delta")
        dS, gS = guarded((B * H * Lq, Lkp), BF16, name="dS") if use_bias else (None, None)
        if dS is not None:
            dS.zero_()
        into = (dq, dk, dv, delta, dS, [g_ for g_ in (gq, gk, gv, gD, gS) if g_ is not None])
        backward(phase=1, into=into)
        assert torch.equal(dq, got[0]) and torch.equal(delta, got[3])
        assert bool((dk.view(torch.int16) == SENTINEL[BF16]).all()) and bool((dv.view(torch.int16) == SENTINEL[BF16]).all())
        backward(phase=2, into=into)
        assert torch.equal(dk, got[1]) and torch.equal(dv, got[2]) and torch.equal(dq, got[0]) and torch.equal(delta, got[3])
    return got


ATTN_GEOMETRIES = {
    # form 0: the short text self-attentions, key mask
    "self8": dict(B=2, Bkv=2, H=2, Lq=8, Lk=8, use_mask=True, seed=210),
    "self30": dict(B=2, Bkv=2, H=2, Lq=30, Lk=30, use_mask=True, seed=200),
    # form 1: one pass per (sequence, head), bias
    "vision65": dict(B=2, Bkv=2, H=2, Lq=65, Lk=65, use_bias=True, seed=500),
    "vision208": dict(B=2, Bkv=2, H=2, Lq=208, Lk=208, use_bias=True, seed=120),
    # form 2: rows sharing K/V
    "cross30x70": dict(B=11, Bkv=2, H=2, Lq=30, Lk=70, use_mask=True, kv_map=[0] * 9 + [1] * 2, seed=330),
    "cross8x5": dict(B=4, Bkv=2, H=2, Lq=8, Lk=5, kv_map=[1, 0, 1, 1], seed=310),
    "cross_unused_image": dict(B=4, Bkv=3, H=2, Lq=30, Lk=70, use_mask=True, kv_map=[0, 2, 2, 0], seed=320),
    # form 3: the long one pass, dQ partials through a workspace of exactly the documented size
    "long209": dict(B=2, Bkv=2, H=2, Lq=209, Lk=209, use_bias=True, seed=700),
    "long272": dict(B=1, Bkv=1, H=2, Lq=272, Lk=272, use_bias=True, seed=710),
    # the two-workgroup resident forward
    "keys230": dict(B=1, Bkv=1, H=2, Lq=230, Lk=230, use_bias=True, seed=130),
    # past the long limits: the streamed pair
    "past641x769": dict(B=1, Bkv=1, H=1, Lq=641, Lk=769, use_bias=True, seed=820),
}
ONE_PASS = [n for n, g in ATTN_GEOMETRIES.items() if expected_form(g["Lq"], g["Lk"], "kv_map" in g, g.get("use_bias", False)) != 0]


@pytest.mark.parametrize("name", list(ATTN_GEOMETRIES))
def test_attention_extents(K, lib, name):
    """LSE: the float32 restatement of the header's formula is within LSE_F32_ERR = 1.21e-6 of float64 on these inputs (measured on the CPU); the device is
    held to LSE_BOUND = 8 x that = 9.68e-6 absolute.  Delta: 1e-5 of max-abs against rowsum(dO * O) of the bf16 tensors handed in."""
    got = run_attention_extents(K, lib, **ATTN_GEOMETRIES[name])
    g = ATTN_GEOMETRIES[name]
    assert got[6] == expected_form(g["Lq"], g["Lk"], "kv_map" in g, g.get("use_bias", False))


@pytest.mark.parametrize("name", ONE_PASS)
def test_attention_extents_two_kernels_where_one_pass_applies(K, lib, name):
    with tuned({14: 1}):
        run_attention_extents(K, lib, **ATTN_GEOMETRIES[name])


@pytest.mark.parametrize("name", ["long209", "long272"])
def test_attention_long_workspace_one_float_short(K, lib, name):
    """X2AttnArgs.ws "NULL / smaller: such a geometry runs the two kernels": one float fewer than B * H * ceil(Lq / 128) * 8192 -> x2_attn_bwd_one_pass
    answers 0, the pair's results are right and the short workspace is not touched"""
    got = run_attention_extents(K, lib, short_ws=True, **ATTN_GEOMETRIES[name])
    assert got[6] == 0


@pytest.mark.parametrize("L", [17, 128])
def test_attention_mask2d_extents(K, L):
    B, H = 3, 2
    r = attn_case(B, B, H, L, L, False, False, None, 900 + L, mask2d=True)
    Lp = K.round_up(L, 64)
    m2 = torch.zeros(B * L, Lp); m2[:, :L] = r["m2"].reshape(B * L, L)
    m2d = filled(m2)
    qd, kd, vd, dod = (seq3(r[n], H, L) for n in ("q", "k", "v", "do"))
    od, gO = out3(B, L, H, "Out")
    lse, gL = guarded((B * H * L,), F32, tail=H * L, name="LSE")
    a = attn_struct(K, B, B, H, L, L, r["scale"], Q=qd, K=kd, V=vd, Out=od, LSE=lse)
    K.call("x2_attn_fwd_mask2d", C.byref(a), m2d.data_ptr(), Lp)
    all_ok(gO, gL)
    e_lse = float((lse.cpu().double() - r["lse"]).abs().max())
    print("mask2d L=%d: out %.2e lse %.2e" % (L, relerr(od, r["out"]), e_lse))
    assert relerr(od, r["out"]) < 6e-3 and e_lse <= LSE_BOUND
    (dq, gq), (dk, gk), (dv, gv) = out3(B, L, H, "dQ"), out3(B, L, H, "dK"), out3(B, L, H, "dV")
    delta, gD = guarded((B * H * L,), F32, tail=H * L, name="Delta")
    a = attn_struct(K, B, B, H, L, L, r["scale"], Q=qd, K=kd, V=vd, O=od, dO=dod, dQ=dq, dK=dk, dV=dv, LSE=lse, Delta=delta)
    K.call("x2_attn_bwd_mask2d", C.byref(a), m2d.data_ptr(), Lp)
    all_ok(gq, gk, gv, gD, gL, gO)
    want_delta = (dod.float().cpu().double() * od.float().cpu().double()).reshape(B, L, H, 64).sum(-1).permute(0, 2, 1).reshape(-1)
    assert max(relerr(dq, r["dq"]), relerr(dk, r["dk"]), relerr(dv, r["dv"])) < 1.5e-2 and relerr(delta, want_delta) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. row-wise kernels

def untouched(view, rows):
    """the listed rows of a guarded interior still hold the sentinel (rows a kernel documents as skipped)"""
    if not isinstance(rows, slice) and len(rows) == 0:
        return True
    return bool((view.view(_INT_OF[view.dtype])[rows] == SENTINEL[view.dtype]).all())


def ln_case(rows, D, period, seed):
    per = period if period else rows
    total = rows if period == 0 else ceil_div(rows, period) * (period + 1)
    x = rnd(total, D, seed=seed, scale=2.0) + 0.5
    w, b = rnd(D, seed=seed + 1) * 0.1 + 1, rnd(D, seed=seed + 2) * 0.1
    sel = torch.arange(rows) if period == 0 else torch.tensor([r + r // period + 1 for r in range(rows)])
    skip = torch.tensor(sorted(set(range(total)) - set(sel.tolist())), dtype=torch.long)
    xs = x.double()[sel]
    mu = xs.mean(1)
    rs = 1.0 / torch.sqrt(xs.var(1, unbiased=False) + 1e-6)
    y = (xs - mu[:, None]) * rs[:, None] * w.double() + b.double()
    return total, x, w, b, sel, skip, mu, rs, y


@pytest.mark.parametrize("period", [0, 4])
@pytest.mark.parametrize("D", [8, 132, 1000, 1540])
@pytest.mark.parametrize("rows", [1, 5, 17])
def test_layernorm_fwd_extents(K, lib, rows, D, period):
    total, x, w, b, sel, skip, mu, rs, y = ln_case(rows, D, period, seed=rows * D)
    xd, wd, bd = filled(x), filled(w), filled(b)
    for knob in (1, 2, 4, 0):
        with tuned({13: knob}):
            (yb, gB), (yf, gF) = guarded((total, D), BF16, name="y_bf16"), guarded((total, D), F32, name="y_f32")
            (mean, gM), (rstd, gR) = guarded((rows,), F32, tail=rows, name="mean"), guarded((rows,), F32, tail=rows, name="rstd")
            K.call("x2_layernorm_fwd", K.ptr(xd), K.ptr(wd), K.ptr(bd), K.ptr(yb), K.ptr(yf), K.ptr(mean), K.ptr(rstd), rows, D, 1e-6, period, 0, 0, 1.0, None)
            all_ok(gB, gF, gM, gR)
            assert relerr(yf[sel.to(dev)], y) < 1e-5 and relerr(yb[sel.to(dev)], y) < 6e-3, knob
            assert relerr(mean, mu) < 1e-5 and relerr(rstd, rs) < 1e-5, knob
            assert untouched(yb, skip.to(dev)) and untouched(yf, skip.to(dev)), knob      # the cls rows (and the rows past the last one) are not written


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("period", [0, 4])
@pytest.mark.parametrize("D", [8, 132, 1000, 1540])
@pytest.mark.parametrize("rows", [1, 5, 17])
def test_layernorm_bwd_extents(K, rows, D, period, defer):
    total, x, w, b, sel, skip, mu, rs, _ = ln_case(rows, D, period, seed=rows * D)
    mean32, rstd32 = mu.float(), rs.float()
    dy, dres = rnd(total, D, seed=7), rnd(total, D, seed=8)
    rowscale = (torch.rand(total, generator=torch.Generator().manual_seed(9)) > 0.2).float() * 1.25
    xd, wd, md, rd, dresd = filled(x), filled(w), filled(mean32), filled(rstd32), filled(dres)
    nblk = ceil_div(rows, 16)

    def reference(dyv):
        xhat = (x.double()[sel] - mean32.double()[:, None]) * rstd32.double()[:, None]
        dyw = dyv.double()[sel] * w.double()
        g = rstd32.double()[:, None] * (dyw - dyw.mean(1, keepdim=True) - xhat * (dyw * xhat).mean(1, keepdim=True))
        return g, (dyv.double()[sel] * xhat).sum(0), dyv.double()[sel].sum(0)

    # (dy dtype, dres, dx, dx_bf16, dcol, post, post rowscale)
    modes = [("f32", True, True, True, False, 0, False), ("bf16", True, True, False, False, 0, False), ("f32", False, True, False, True, 0, False)]
    if period == 0:
        modes += [("bf16", True, True, True, True, 1, False), ("bf16", True, True, True, True, 1, True)]
    selg, skipg = sel.to(dev), skip.to(dev)
    for dyt, use_dres, want_dx, want_bf, use_dcol, post, use_rs in modes:
        dyv = dy if dyt == "f32" else bf(dy)
        g, dw_ref, db_ref = reference(dyv)
        dyd = filled(dyv)
        (dx, gX), (dxb, gXb) = guarded((total, D), F32, name="dx"), guarded((total, D), BF16, name="dx_bf16")
        (dw, gW), (db, gB), (dcol, gC) = (guarded((D,), F32, tail=D, name=n) for n in ("dw", "db", "dcol"))
        for t in (dw, db, dcol):
            t.fill_(0.5)
        ws, gS = guarded((nblk * 3 * D,), F32, tail=3 * D, name="ws")
        rsd = filled(rowscale) if use_rs else None
        K.call("x2_layernorm_bwd", K.ptr(dyd), 1 if dyt == "bf16" else 0, K.ptr(xd), K.ptr(md), K.ptr(rd), K.ptr(wd), K.ptr(dresd) if use_dres else None,
               K.ptr(dx), K.ptr(dxb) if want_bf else None, K.ptr(dw), K.ptr(db), K.ptr(dcol) if use_dcol else None, rows, D, period, 0, 0, 1.0, 0, 0, 1.0,
               None, K.ptr(ws), defer, post, K.ptr(rsd))
        if defer:
            all_ok(gW, gB, gC)
            assert float(dw.min()) == 0.5 and float(dw.max()) == 0.5                 # stage 1 alone adds nothing yet
            K.call("x2_reduce_partials", K.ptr(ws), nblk, 3, D, K.ptr(dw), K.ptr(db), K.ptr(dcol) if use_dcol else None)
        all_ok(gX, gXb, gW, gB, gC, gS)
        mode = (dyt, use_dres, use_dcol, post, use_rs)
        full = g + (dres.double()[sel] if use_dres else 0.0)
        assert relerr(dx[selg], full) < 2e-5, mode
        assert untouched(dx, skipg), mode
        assert relerr(dw - 0.5, dw_ref) < 2e-5 and relerr(db - 0.5, db_ref) < 2e-5, mode
        if not use_dcol:
            assert float(dcol.min()) == 0.5 and float(dcol.max()) == 0.5, mode
        if want_bf:
            want_b = full * (rowscale.double()[sel][:, None] if use_rs else 1.0) if post else g
            assert relerr(dxb[selg], want_b) < 6e-3 and untouched(dxb, skipg), mode
        else:
            assert untouched(dxb, slice(None)), mode
        if use_dcol:
            want_c = (full * (rowscale.double()[sel][:, None] if use_rs else 1.0)).sum(0) if post else g.sum(0)
            assert relerr(dcol - 0.5, want_c) < 5e-5, mode


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("N", [8, 520])
@pytest.mark.parametrize("M", [1, 63, 65])
def test_colsum_bf16_extents(K, M, N, defer):
    y = bf(rnd(M, N, seed=M + N))
    yd = filled(y, ld=N + 8)
    nblk = ceil_div(M, 64)
    ws, gS = guarded((nblk * N,), F32, tail=N, name="ws")
    out, gO = guarded((N,), F32, tail=N, name="out")
    out.fill_(2.0)
    K.call("x2_colsum_bf16", K.ptr(yd), K.ptr(out), M, N, N + 8, K.ptr(ws), defer)
    if defer:
        all_ok(gO)
        assert float(out.min()) == 2.0 and float(out.max()) == 2.0
        K.call("x2_reduce_partials", K.ptr(ws), nblk, 1, N, K.ptr(out), None, None)
    all_ok(gS, gO)
    assert relerr(out - 2.0, y.double().sum(0)) < 1e-5


@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("D", [4, 260])
@pytest.mark.parametrize("M", [1, 31, 33])
def test_rowscale_cast_colsum_extents(K, M, D, defer):
    dx = rnd(M, D, seed=M + D)
    rs = (torch.rand(M, generator=torch.Generator().manual_seed(3)) > 0.2).float() * 1.25
    dxd, nblk = filled(dx), ceil_div(M, 32)
    for rowscale in (None, rs):
        ws, gS = guarded((nblk * D,), F32, tail=D, name="ws")
        cs, gC = guarded((D,), F32, tail=D, name="colsum")
        dxb, gB = guarded((M, D), BF16, name="dx_bf16")
        cs.fill_(1.0)
        K.call("x2_rowscale_cast_colsum", K.ptr(dxd), K.ptr(filled(rowscale)) if rowscale is not None else None, K.ptr(dxb), K.ptr(cs), M, D, K.ptr(ws), defer)
        if defer:
            K.call("x2_reduce_partials", K.ptr(ws), nblk, 1, D, K.ptr(cs), None, None)
        all_ok(gS, gC, gB)
        want = dx if rowscale is None else dx * rowscale[:, None]
        assert torch.equal(dxb.cpu(), bf(want)) and relerr(cs - 1.0, want.double().sum(0)) < 1e-5


@pytest.mark.parametrize("width", [8, 30, 65, 100])
def test_reduce_partials_extents(K, width):
    """x2_reduce_partials (nk <= 3) and x2_reduce_partials_multi (nk <= 4, several reductions in one launch), a null output slot in each"""
    nblk = 7
    part = rnd(nblk, 3, width, seed=width)
    outs = [guarded((width,), F32, tail=width, name="o%d" % k) for k in range(3)]
    for o, _ in outs:
        o.fill_(1.0)
    K.call("x2_reduce_partials", K.ptr(filled(part.reshape(-1))), nblk, 3, width, K.ptr(outs[0][0]), None, K.ptr(outs[2][0]))
    all_ok(*(g for _, g in outs))
    for k in (0, 2):
        assert relerr(outs[k][0] - 1.0, part[:, k].double().sum(0)) < 1e-5
    assert float(outs[1][0].min()) == 1.0 and float(outs[1][0].max()) == 1.0
    items, flat, keep = [], [], []
    for i, (nb, nk) in enumerate(((5, 4), (1, 1), (13, 2))):
        p = rnd(nb, nk, width, seed=100 + i)
        pd = filled(p.reshape(-1))
        os_ = [None if (nk == 4 and k == 1) else guarded((width,), F32, tail=width, name="multi o%d" % k) for k in range(nk)]
        for o in os_:
            if o is not None:
                o[0].fill_(float(i))
        keep.append(pd)
        items.append((p, os_, i))
        flat += [pd.data_ptr(), nb, nk, width] + [0 if o is None else o[0].data_ptr() for o in os_] + [0] * (4 - nk)
    K.call("x2_reduce_partials_multi", (C.c_int64 * len(flat))(*flat), len(items))
    for p, os_, i in items:
        for k, o in enumerate(os_):
            if o is not None:
                all_ok(o[1])
                assert relerr(o[0] - float(i), p[:, k].double().sum(0)) < 1e-5


@pytest.mark.parametrize("N,Kd", [(5, 12), (9, 260)])
def test_layerscale_finish_extents(K, N, Kd):
    G, W, b, gamma, cs = rnd(N, Kd, seed=1), rnd(N, Kd, seed=2), rnd(N, seed=3), rnd(N, seed=4) * 0.3 + 0.1, rnd(N, seed=5)
    for with_bias in (True, False):
        Gd, gG = guarded((N, Kd), F32, name="G")
        Gd.copy_(G)
        (dg, gD), (dbias, gB) = guarded((N,), F32, tail=N, name="dgamma"), guarded((N,), F32, tail=N, name="dbias")
        dg.fill_(2.0); dbias.fill_(3.0)
        Wd, bd, gd, csd = filled(W), filled(b), filled(gamma), filled(cs)
        desc = [Gd.data_ptr(), Wd.data_ptr(), bd.data_ptr() if with_bias else 0, gd.data_ptr(), csd.data_ptr(), dg.data_ptr(), dbias.data_ptr() if with_bias else 0, N, Kd]
        K.call("x2_layerscale_finish", (C.c_int64 * 9)(*desc), 1)
        all_ok(gG, gD, gB)
        want_dg = (G.double() * W.double()).sum(1) + (b.double() * cs.double() if with_bias else 0.0)
        assert relerr(dg - 2.0, want_dg) < 1e-5 and relerr(Gd, G.double() * gamma.double()[:, None]) < 1e-5
        if with_bias:
            assert relerr(dbias - 3.0, gamma.double() * cs.double()) < 1e-5
        else:
            assert float(dbias.min()) == 3.0 and float(dbias.max()) == 3.0


@pytest.mark.parametrize("R,Cc", [(4, 4), (68, 132)])
def test_cast_transpose_extents(K, R, Cc):
    """dst [R][C]; dstT [C][ldt] with ldt > R: columns R .. ldt - 1 are left untouched (a row gap here).  The multi form writes rows roff .. of dst and
    columns roff .. of dstT, with and without a row scale on the transposed copy."""
    src, ldt = rnd(R, Cc, seed=R), R + 4
    srcd = filled(src)
    (d, gD), (dT, gT) = guarded((R, Cc), BF16, name="dst"), guarded((Cc, R), BF16, ld=ldt, name="dstT")
    K.call("x2_cast_transpose_bf16", K.ptr(srcd), K.ptr(d), K.ptr(dT), R, Cc, ldt)
    all_ok(gD, gT)
    assert torch.equal(d.cpu(), bf(src)) and torch.equal(dT.cpu(), bf(src).t())
    dT, gT = guarded((Cc, R), BF16, ld=ldt, name="dstT alone")
    K.call("x2_cast_transpose_bf16", K.ptr(srcd), None, K.ptr(dT), R, Cc, ldt)
    all_ok(gT)
    assert torch.equal(dT.cpu(), bf(src).t())
    roff, ts = 4, rnd(R, seed=9)
    for tscale in (None, ts):
        (d, gD), (dT, gT) = guarded((R, Cc), BF16, name="dst rows roff.."), guarded((Cc, R), BF16, ld=roff + R + 4, name="dstT columns roff..")
        desc = [srcd.data_ptr(), d.data_ptr() - 2 * roff * Cc, dT.data_ptr() - 2 * roff, R, Cc, roff + R + 4, roff, 0 if tscale is None else filled(tscale).data_ptr()]
        K.call("x2_cast_transpose_multi", (C.c_int64 * 8)(*desc), 1)
        all_ok(gD, gT)
        assert torch.equal(d.cpu(), bf(src)) and torch.equal(dT.cpu(), bf(src if tscale is None else src * tscale[:, None]).t())


def relpos_index(window):
    from oracle import x2vlm_oracle as O
    return O.relative_position_index(window)


@pytest.mark.parametrize("window", [2, 4], ids=["N5", "N17"])
def test_relpos_bias_extents(K, window):
    idx = relpos_index(window)
    N, H, T = idx.shape[0], 3, int(idx.max()) + 1
    table = rnd(T, H, seed=5)
    ld, ldT = 64, 128
    (bias, gB), (biasT, gT) = guarded((H * N, ld), F32, name="bias"), guarded((H * N, ldT), F32, name="biasT")
    K.call("x2_relpos_bias", K.ptr(filled(table)), K.ptr(filled(idx)), K.ptr(filled(idx.t().contiguous())), K.ptr(bias), K.ptr(biasT), N, H, ld, ldT, 1.0)
    all_ok(gB, gT)
    ref = table[idx.reshape(-1)].view(N, N, H).permute(2, 0, 1)
    b, bT = bias.view(H, N, ld).cpu(), biasT.view(H, N, ldT).cpu()
    assert torch.equal(b[..., :N], ref) and torch.equal(bT[..., :N], ref.transpose(1, 2))
    assert float(b[..., N:].abs().max()) == 0.0 and float(bT[..., N:].abs().max()) == 0.0          # the documented zeros in the pad columns
    bias, gB = guarded((H * N, ld), F32, name="bias alone")
    K.call("x2_relpos_bias", K.ptr(filled(table)), K.ptr(filled(idx)), None, K.ptr(bias), None, N, H, ld, ld, 1.0)
    all_ok(gB)
    assert torch.equal(bias.view(H, N, ld).cpu()[..., :N], ref)


@pytest.mark.parametrize("slices", [1, 2])
@pytest.mark.parametrize("window", [2, 4], ids=["N5", "N17"])
def test_relpos_bias_bwd_extents(K, window, slices):
    idx = relpos_index(window)
    N, H, B, ld = idx.shape[0], 3, 2, 64
    T = int(idx.max()) + 1
    dS = bf(rnd(B, H, N, ld, seed=6))
    dS[..., N:] = 0
    dS[..., ceil_div(N, 8) * 8:] = float("nan")         # "reads columns j < 8 ceil(N / 8) of dS only"
    flat = idx.reshape(-1)
    order = torch.argsort(flat, stable=True)
    off = torch.zeros(T + 1, dtype=I32); off[1:] = torch.cumsum(torch.bincount(flat, minlength=T), 0)
    pos = ((order // N) * ld + order % N).to(I32)
    dtab, gD = guarded((T, H), F32, name="dtable")
    dtab.fill_(1.0)
    ws, gS = guarded((slices * H * N * ld,), F32, tail=H * N * ld, name="ws")
    K.call("x2_relpos_bias_bwd", K.ptr(filled(dS.reshape(-1, ld))), K.ptr(filled(off)), K.ptr(filled(pos)), K.ptr(dtab), B, N, H, ld, T, K.ptr(ws), slices)
    all_ok(gD, gS)
    ref = torch.ones(T, H, dtype=torch.float64).index_add_(0, flat, dS[..., :N].double().sum(0).permute(1, 2, 0).reshape(-1, H))
    assert relerr(dtab, ref) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. heads and embeddings

def mlm_inputs(R, Hd=64, V=100, Vp=128):
    x = bf(rnd(R, Hd, seed=21 + R))
    E = torch.zeros(Vp, Hd); E[:V] = rnd(V, Hd, seed=22, scale=3.0 * Hd ** -0.5)
    bias = torch.zeros(Vp); bias[:V] = rnd(V, seed=23)
    labels = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(24 + R))
    labels[::5] = -100
    labels[R // 2] = V - 1                       # last valid column, in the chunk that also holds the padding
    E = bf(E)
    z = x.double() @ E.double().t()[:, :V] + bias[:V].double()
    return x, E, bias, labels, z


@pytest.mark.parametrize("R", [1, 37, 65, 129])
def test_mlm_ce_extents(K, R):
    Hd, V, Vp, ldd = 64, 100, 128, 128 + 64
    x, E, bias, labels, z = mlm_inputs(R)
    if R == 1:
        labels[0] = 7
    xd, Ed, bd, ld = filled(x, ld=Hd + 8), filled(E, ld=Hd + 8), filled(bias), filled(labels)
    (part, gP), (zlab, gZ) = guarded((R * (Vp // 64) * 2,), F32, tail=2 * (Vp // 64), name="part"), guarded((R,), F32, tail=R, name="zlab")
    K.call("x2_mlm_ce_fwd", K.ptr(xd), K.ptr(Ed), K.ptr(bd), K.ptr(ld), R, Vp, V, Hd, Hd + 8, Hd + 8, K.ptr(part), K.ptr(zlab))
    all_ok(gP, gZ)
    (lse, gL), (rows, gR), (out2, g2) = guarded((R,), F32, tail=R, name="lse"), guarded((R,), F32, tail=R, name="loss_row"), guarded((2,), F32, tail=2, name="out2")
    K.call("x2_ce_combine", K.ptr(part), Vp // 64, K.ptr(zlab), K.ptr(ld), R, K.ptr(lse), K.ptr(rows), K.ptr(out2))
    all_ok(gP, gZ, gL, gR, g2)
    valid = labels >= 0
    ref_lse = torch.logsumexp(z, -1)
    ref_rows = (ref_lse - z[torch.arange(R), labels.clamp_min(0)]) * valid
    assert float((lse.cpu().double() - ref_lse).abs().max()) < 1e-4
    assert float((rows.cpu().double() - ref_rows).abs().max()) < 1e-4 and float(rows.cpu()[~valid].abs().sum()) == 0.0
    mean = float(ref_rows.sum() / valid.sum())
    assert abs(float(out2[0]) - mean) < 1e-5 * max(1.0, mean) and float(out2[1]) == float(valid.sum())
    dl, gD = guarded((R, Vp), BF16, ld=ldd, name="dl")
    K.call("x2_mlm_ce_bwd", K.ptr(xd), K.ptr(Ed), K.ptr(bd), K.ptr(ld), K.ptr(lse), K.ptr(filled(torch.tensor([0.7]))), K.ptr(out2), 1.0, R, Vp, V, Hd, Hd + 8, Hd + 8,
           K.ptr(dl), ldd)
    all_ok(gD, gL, g2)
    ref_dl = torch.softmax(z, -1)
    ref_dl[torch.arange(R), labels.clamp_min(0)] -= 1.0
    ref_dl = ref_dl * (0.7 / float(valid.sum())) * valid.double().unsqueeze(1)
    assert relerr(dl[:, :V], ref_dl) < 6e-3
    assert float(dl[:, V:].float().abs().max()) == 0.0 and (bool(valid.all()) or float(dl[(~valid).to(dev)].float().abs().max()) == 0.0)


@pytest.mark.parametrize("R", [1, 37, 65, 129])
def test_mlm_ls_extents(K, R):
    Hd, V, Vp, ldd, ignore, ls = 64, 100, 128, 128 + 64, 2, 0.1
    x, E, bias, labels, z = mlm_inputs(R)
    labels[labels < 0] = ignore
    if R == 1:
        labels[0] = 7
    w = torch.ones(R); w[labels == ignore] = 0.0
    if R > 3:
        w[3] = 0.0
    xd, Ed, bd, ld, wd = filled(x, ld=Hd + 8), filled(E, ld=Hd + 8), filled(bias), filled(labels), filled(w)
    nch = Vp // 64
    (part, gP), (sumz, gS) = guarded((R * nch * 2,), F32, tail=2 * nch, name="part"), guarded((R * nch,), F32, tail=nch, name="sumz")
    (zlab, gZ), (zign, gI) = guarded((R,), F32, tail=R, name="zlab"), guarded((R,), F32, tail=R, name="zign")
    K.call("x2_mlm_ls_fwd", K.ptr(xd), K.ptr(Ed), K.ptr(bd), K.ptr(ld), ignore, R, Vp, V, Hd, Hd + 8, Hd + 8, K.ptr(part), K.ptr(sumz), K.ptr(zlab), K.ptr(zign))
    all_ok(gP, gS, gZ, gI)
    (lse, gL), (rows, gR), (out2, g2) = guarded((R,), F32, tail=R, name="lse"), guarded((R,), F32, tail=R, name="kl_row"), guarded((2,), F32, tail=2, name="out2")
    K.call("x2_ls_combine", K.ptr(part), K.ptr(sumz), nch, K.ptr(zlab), K.ptr(zign), K.ptr(ld), K.ptr(wd), R, V, ignore, ls, K.ptr(lse), K.ptr(rows), K.ptr(out2))
    all_ok(gP, gS, gZ, gI, gL, gR, g2)
    zl = z.clone().requires_grad_(True)
    q = torch.full((R, V), ls / (V - 2), dtype=torch.float64)
    q[:, ignore] = 0
    q.scatter_(1, labels.view(-1, 1), 1.0 - ls)
    q[labels == ignore] = 0
    kl = torch.nn.functional.kl_div(torch.log_softmax(zl, -1), q, reduction="none").sum(-1)
    loss = (kl * w.double() / (w.double().sum() + 1e-5)).sum()
    loss.backward()
    assert float((lse.cpu().double() - torch.logsumexp(z, -1)).abs().max()) < 1e-4
    assert abs(float(out2[0]) - float(loss)) / max(1.0, abs(float(loss))) < 1e-6 and float(out2[1]) == float(w.sum())
    dl, gD = guarded((R, Vp), BF16, ld=ldd, name="dl")
    K.call("x2_mlm_ls_bwd", K.ptr(xd), K.ptr(Ed), K.ptr(bd), K.ptr(ld), K.ptr(wd), K.ptr(lse), K.ptr(filled(torch.tensor([0.7]))), K.ptr(out2), 1.0, ls, ignore,
           R, Vp, V, Hd, Hd + 8, Hd + 8, K.ptr(dl), ldd)
    all_ok(gD, gL, g2)
    if float(w.sum()) > 0:
        assert relerr(dl[:, :V], zl.grad * 0.7) < 6e-3
    dead = (labels == ignore) | (w == 0)
    assert float(dl[:, V:].float().abs().max()) == 0.0 and (not bool(dead.any()) or float(dl[dead.to(dev)].float().abs().max()) == 0.0)


@pytest.mark.parametrize("pid", [False, True], ids=["embed_bwd", "embed_bwd_pid"])
@pytest.mark.parametrize("D", [8, 132, 1536])
@pytest.mark.parametrize("R,L", [(3, 8), (96, 8)])
def test_embed_bwd_extents(K, R, L, D, pid):
    """scratch of exactly min(L, R) * D floats; dtype0 is row 0 of a [2][D] buffer whose row 1 (the trailing guard here) must survive"""
    V, P = 7, 11
    g_ = torch.Generator().manual_seed(R + D)
    ids = torch.randint(0, V, (R,), generator=g_)
    pids = torch.randint(0, P, (R,), generator=g_) if pid else torch.arange(R) % L
    gr = rnd(R, D, seed=D)
    Lp = min(L, R)
    (dword, gW), (dtype0, gT) = guarded((V, D), F32, name="dword"), guarded((D,), F32, tail=D, name="dtype0")
    dpos, gP = guarded((P if pid else Lp, D), F32, name="dpos")
    scratch, gS = guarded((Lp * D,), F32, tail=D, name="scratch")
    for t in (dword, dpos, dtype0):
        t.fill_(0.25)
    if pid:
        K.call("x2_embed_bwd_pid", K.ptr(filled(ids)), K.ptr(filled(pids)), K.ptr(filled(gr)), K.ptr(dword), K.ptr(dpos), K.ptr(dtype0), R, L, D, K.ptr(scratch))
    else:
        K.call("x2_embed_bwd", K.ptr(filled(ids)), K.ptr(filled(gr)), K.ptr(dword), K.ptr(dpos), K.ptr(dtype0), R, L, D, K.ptr(scratch))
    all_ok(gW, gT, gP, gS)
    rw = torch.full((V, D), 0.25, dtype=torch.float64).index_add_(0, ids, gr.double())
    rp = torch.full((dpos.shape[0], D), 0.25, dtype=torch.float64).index_add_(0, pids, gr.double())
    assert relerr(dword, rw) < 1e-5 and relerr(dpos, rp) < 1e-5 and relerr(dtype0, 0.25 + gr.double().sum(0)) < 1e-5


# ------------------------------------------------------------------------------------------------ 2. glue kernels that build index tables

def test_kv_csr_extents(K):
    S, Bi = 11, 4
    kv = torch.tensor([3, 0, 0, 2, 3, 3, 0, 2, 0, 3, 0], dtype=I32)             # K/V batch 1 is used by nobody
    (off, gO), (order, gR) = guarded((Bi + 1,), I32, name="off"), guarded((S,), I32, name="order")
    K.call("x2_kv_csr", K.ptr(filled(kv)), S, Bi, K.ptr(off), K.ptr(order))
    all_ok(gO, gR)
    want_off = torch.zeros(Bi + 1, dtype=I32); want_off[1:] = torch.cumsum(torch.bincount(kv, minlength=Bi), 0)
    assert torch.equal(off.cpu(), want_off) and torch.equal(order.cpu(), torch.argsort(kv, stable=True).to(I32))


@pytest.mark.parametrize("with_match", [1, 0])
def test_tail_index_extents(K, with_match):
    g = torch.Generator().manual_seed(5)
    B, Bi, L, T = 3, 3, 5, 7
    ineg, tneg = torch.randint(0, B, (B,), generator=g, dtype=I32), torch.randint(0, B, (B,), generator=g, dtype=I32)
    ta, ia = (torch.rand(B, L, generator=g) > 0.3).long(), (torch.rand(Bi, T, generator=g) > 0.2).long()
    R = 4 * B if with_match else B
    (t_idx, g1), (kv, g2) = guarded((R,), I32, name="t_idx"), guarded((R,), I32, name="kv")
    (atts, g3), (enc, g4) = guarded((R, L), I64, name="atts_out"), guarded((R, T), I64, name="enc_out")
    K.call("x2_tail_index", K.ptr(filled(ineg)) if with_match else None, K.ptr(filled(tneg)) if with_match else None, K.ptr(filled(ta)), K.ptr(filled(ia)), B, L, T,
           with_match, K.ptr(t_idx), K.ptr(kv), K.ptr(atts), K.ptr(enc))
    all_ok(g1, g2, g3, g4)
    ar = torch.arange(B, dtype=I32)
    ti = torch.cat([ar, ar, tneg, ar + B]) if with_match else ar + B
    ki = torch.cat([ar, ineg, ar, ar]) if with_match else ar
    assert torch.equal(t_idx.cpu(), ti) and torch.equal(kv.cpu(), ki)
    assert torch.equal(atts.cpu(), torch.cat([ta, ta])[ti.long()]) and torch.equal(enc.cpu(), ia[ki.long()])


def test_additive_masks_extents(K):
    """out [S][Lp] / [S][L][Lp] guarded; the pad columns L .. Lp - 1 hold the documented zeros"""
    g = torch.Generator().manual_seed(6)
    S, L, Lp = 3, 5, 64
    atts = (torch.rand(S, L, generator=g) > 0.3).long()
    out, gO = guarded((S, Lp), F32, name="mask")
    K.call("x2_additive_mask", K.ptr(filled(atts)), K.ptr(out), S, L, Lp, -10000.0)
    all_ok(gO)
    assert torch.equal(out[:, :L].cpu(), (1.0 - atts.float()) * -10000.0) and float(out[:, L:].abs().max()) == 0.0
    for L2, Lp2 in ((5, 64), (65, 128)):
        m = (torch.rand(S, L2, L2, generator=g) > 0.3).long()
        out, gO = guarded((S * L2, Lp2), F32, name="mask2d")
        K.call("x2_additive_mask2d", K.ptr(filled(m.reshape(-1))), K.ptr(out), S, L2, Lp2, -10000.0)
        all_ok(gO)
        assert torch.equal(out[:, :L2].cpu(), (1.0 - m.float().reshape(S * L2, L2)) * -10000.0) and float(out[:, L2:].abs().max()) == 0.0


def test_mask_tokens_extents(K):
    import numpy as np
    from oracle import masking_oracle as mo
    B, L, V, MM = 5, 13, 200, 6
    rng = np.random.default_rng(17)
    sub = (np.arange(V) % 3 == 0).astype(np.uint8); sub[:8] = 0
    ids = np.zeros((B, L), dtype=np.int64); atts = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        n = int(rng.integers(2, L + 1)) if b else L
        ids[b, :n] = rng.integers(8, V, size=n); ids[b, 0] = 1; ids[b, n - 1] = 2; atts[b, :n] = 1
    words = rng.integers(0, 1 << 32, size=(B, 4 * L + 64), dtype=np.uint64).astype(np.uint32)
    kw = dict(mask_prob=0.5, max_masks=MM, skipgram_prb=0.2, skipgram_size=3, mask_whole_word=True, cls_id=1, mask_id=3)
    want = mo.mask_tokens(ids, atts, sub, words, vocab_size=V, **kw)
    (idm, g1), (mpos, g2), (mids, g3) = guarded((B, L), I64, name="text_ids_masked"), guarded((B, MM), I64, name="masked_pos"), guarded((B, MM), I64, name="masked_ids")
    wd = filled(torch.from_numpy(words.view(np.int32)))
    K.call("x2_mask_tokens", K.ptr(filled(torch.from_numpy(ids))), K.ptr(filled(torch.from_numpy(atts))), B, L, K.ptr(torch.from_numpy(sub).to(dev)), V, K.ptr(wd),
           words.shape[1], 0, None, 0.5, MM, 0.2, 3, 1, 1, 3, 0, -100, K.ptr(idm), K.ptr(mpos), K.ptr(mids))
    all_ok(g1, g2, g3)
    for got, w_ in zip((idm, mpos, mids), want):
        assert np.array_equal(got.cpu().numpy(), w_)


def test_droppath_rows_extents(K):
    rates, B, T = [0.0, 0.1, 0.5], 5, 3
    out, gO = guarded((len(rates) * 2 * B * T,), F32, tail=B * T, name="droppath rows")
    K.call("x2_droppath_rows", K.ptr(filled(torch.tensor(rates))), 1234, None, len(rates), B, T, K.ptr(out))
    all_ok(gO)
    rows, keep = out.cpu().view(len(rates), 2, B, T), K.droppath_keep(rates, 1234, B)
    for l, rate in enumerate(rates):
        assert torch.equal(rows[l], (keep[l] / (1.0 - torch.tensor(rate, dtype=F32))).unsqueeze(-1).expand(2, B, T).contiguous()), l


def test_frame_mean_extents(K):
    Bc, F, T, D = 2, 3, 5, 12
    x, pos, dy = rnd(Bc * F, T, D, seed=1), rnd(F, D, seed=2), rnd(Bc, T, D, seed=3)
    out, gO = guarded((Bc * T, D), F32, name="out")
    K.call("x2_frame_mean", K.ptr(filled(x.reshape(-1, D))), K.ptr(filled(pos)), None, K.ptr(out), None, Bc, F, T, D, 0)
    all_ok(gO)
    assert relerr(out.view(Bc, T, D), (x.double().view(Bc, F, T, D) + pos.double().view(1, F, 1, D)).mean(1)) < 1e-5
    (dx, gX), (dpos, gP) = guarded((Bc * F * T, D), F32, name="dx"), guarded((F, D), F32, name="dpos")
    K.call("x2_frame_mean", None, None, K.ptr(filled(dy.reshape(-1, D))), K.ptr(dx), K.ptr(dpos), Bc, F, T, D, 1)
    all_ok(gX, gP)
    assert relerr(dx.view(Bc, F, T, D), (dy.double() / F)[:, None].expand(Bc, F, T, D)) < 1e-5
    assert relerr(dpos, (dy.double().sum((0, 1)) / F)[None].expand(F, D)) < 1e-5


def test_sample_negatives_extents(K):
    n = 5
    sim, u = rnd(n, n, seed=3, scale=2.0), torch.tensor([0.05, 0.3, 0.5, 0.7, 0.95])
    out, gO = guarded((n,), I32, name="picks")
    K.call("x2_sample_negatives", K.ptr(filled(sim.reshape(-1))), n, None, K.ptr(filled(u)), K.ptr(out))
    all_ok(gO)
    w = torch.softmax(sim.double(), 1) + 1e-5
    w.fill_diagonal_(0)
    cdf = torch.cumsum(w, 1)
    target = u.double() * cdf[:, -1]
    ref = (cdf > target.unsqueeze(1)).float().argmax(1)
    assert float((cdf - target[:, None]).abs().min()) > 1e-4          # no draw sits within fp32 rounding of a CDF step: the pick is unambiguous
    assert torch.equal(out.cpu().long(), ref)


# ------------------------------------------------------------------------------------------------ 3. the wrappers' own workspace formulas

@pytest.fixture
def exact_workspace(K, monkeypatch):
    """kernels.workspace() - and the private buffer _ws_and_defer allocates under kernels.DEFERRED - hand out guarded buffers of exactly the size the
    wrapper's formula asks for (behind them: 65536 floats, the largest unit of any workspace layout) -> the list of (view, Guard, nfloats)"""
    handed = []

    def workspace(device, nfloats):
        v, g = guarded((nfloats,), F32, tail=65536, name="workspace(%d)" % nfloats)
        handed.append((v, g, nfloats))
        return v

    monkeypatch.setattr(K, "workspace", workspace)
    monkeypatch.setattr(K, "_ws_and_defer", lambda device, nfloats: (workspace(device, nfloats), 0 if K.DEFERRED is None else 1))
    yield handed
    K.DEFERRED = None


def both_ways(K, handed, run, check):
    """run() inline, then under kernels.DEFERRED with the collected stage-2 reductions launched afterwards; every handed workspace intact"""
    for deferred in (False, True):
        del handed[:]
        K.DEFERRED = [] if deferred else None
        try:
            res = run()
            items, K.DEFERRED = K.DEFERRED, None
            if deferred:
                assert len(items) >= 1
                K.reduce_partials_multi(items)
        finally:
            K.DEFERRED = None
        assert len(handed) >= 1
        all_ok(*(g for _, g, _ in handed))
        check(res)


def test_wrapper_workspaces_of_the_column_reductions(K, exact_workspace):
    M, N, Kd = 193, 136, 128
    A, B, pre = bf(rnd(M, Kd, seed=1)), bf(rnd(N, Kd, seed=2, scale=Kd ** -0.5)), bf(rnd(M, N, seed=3))
    want = (A.double() @ B.double().t()) * dgelu64(pre.double())
    Ad, Bd, pd = A.to(dev), B.to(dev), pre.to(dev)

    def run():
        cs = torch.full((N,), 3.0, device=dev)
        return K.gemm_nt_dgelu_colsum(Ad, Bd, pd, cs), cs

    def check(res):
        assert relerr(res[0], want) < 6e-3 and float((res[1].cpu().double() - 3.0 - want.sum(0)).abs().max()) <= 1e-5 * float(want.abs().sum(0).max()) + 1e-6
    both_ways(K, exact_workspace, run, check)
    assert exact_workspace[-1][2] == 2 * ceil_div(M, 64) * N

    # LayerNorm backward: ceil(rows / 16) * 3 * D
    rows, D = 17, 132
    total, x, w, b, sel, skip, mu, rs, _ = ln_case(rows, D, 0, seed=5)
    dy, dres = rnd(rows, D, seed=7), rnd(rows, D, seed=8)
    xhat = (x.double() - mu.float().double()[:, None]) * rs.float().double()[:, None]
    dyw = dy.double() * w.double()
    g = rs.float().double()[:, None] * (dyw - dyw.mean(1, keepdim=True) - xhat * (dyw * xhat).mean(1, keepdim=True))

    def run():
        dw, db = torch.zeros(D, device=dev), torch.zeros(D, device=dev)
        dx, _ = K.layernorm_bwd(dy.to(dev), x.to(dev), mu.float().to(dev), rs.float().to(dev), w.to(dev), dw, db, dres=dres.to(dev))
        return dx, dw, db

    def check(res):
        assert relerr(res[0], g + dres.double()) < 2e-5 and relerr(res[1], (dy.double() * xhat).sum(0)) < 2e-5 and relerr(res[2], dy.double().sum(0)) < 2e-5
    both_ways(K, exact_workspace, run, check)
    assert exact_workspace[-1][2] == ceil_div(rows, 16) * 3 * D

    y = bf(rnd(65, 520, seed=9))

    def run():
        out = torch.zeros(520, device=dev)
        K.colsum_bf16(y.to(dev), out)
        return out
    both_ways(K, exact_workspace, run, lambda out: relerr(out, y.double().sum(0)) < 1e-5 or pytest.fail("colsum_bf16"))
    assert exact_workspace[-1][2] == 2 * 520

    dx = rnd(33, 260, seed=10)

    def run():
        cs = torch.zeros(260, device=dev)
        return K.rowscale_cast_colsum(dx.to(dev), cs), cs
    both_ways(K, exact_workspace, run, lambda r_: (torch.equal(r_[0].cpu(), bf(dx)) and relerr(r_[1], dx.double().sum(0)) < 1e-5) or pytest.fail("rowscale_cast_colsum"))
    assert exact_workspace[-1][2] == 2 * 260


def test_wrapper_workspaces_of_the_gemms(K, lib, exact_workspace):
    M, N, Kd = 130, 136, 640
    A, B = bf(rnd(M, Kd, seed=11)), bf(rnd(N, Kd, seed=12, scale=Kd ** -0.5))
    ref = A.double() @ B.double().t()
    for slices in (0, 3, 10):
        del exact_workspace[:]
        out = K.gemm_nt_splitk(A.to(dev), B.to(dev), slices=slices)
        all_ok(*(g for _, g, _ in exact_workspace))
        assert relerr(out, ref) < 1e-5 and exact_workspace[-1][2] == min(32, Kd // 64) * M * N
    Mc, N, Kd = 192, 264, 320
    dY, X = bf(rnd(Mc, N, seed=1)), bf(rnd(Mc, Kd, seed=2))
    ref = dY.double().t() @ X.double()
    for tile in (0, 1, 2):
        with tuned({5: tile}):
            for split in (0, 1, 2, 3):
                if split > 1 and tile == 1:
                    continue                      # the 128x128 kernel adds split partials atomically
                del exact_workspace[:]
                dW = torch.full((N, Kd), 7.0, device=dev)
                K.gemm_tn_grouped([(dY.to(dev), X.to(dev), dW)], split=split)
                all_ok(*(g for _, g, _ in exact_workspace))
                assert relerr(dW, ref) < 1e-5, (tile, split)
                assert split == 1 or exact_workspace[-1][2] == (split if split else 4) * 4 * 65536
    # linear_f32 with K slices: ksplit * M * N
    a, b, bias = rnd(33, 200, seed=1), rnd(10, 200, seed=2), rnd(10, seed=3)
    del exact_workspace[:]
    out = K.linear_f32(a.to(dev), b.to(dev), bias=bias.to(dev))
    all_ok(*(g for _, g, _ in exact_workspace))
    assert len(exact_workspace) == 1 and exact_workspace[0][2] == 3 * 33 * 10
    assert relerr(out, a.double() @ b.double().t() + bias.double()) < 1e-5


def test_wrapper_workspaces_of_attention_relpos_embeddings(K, lib, exact_workspace):
    # attn_bwd, form 3: B * H * ceil(Lq / 128) * 8192
    g_ = ATTN_GEOMETRIES["long209"]
    B, H, L = g_["B"], g_["H"], g_["Lq"]
    r = attn_case(B, B, H, L, L, True, False, None, g_["seed"])
    Lkp, Lqp = K.round_up(L, 64), K.round_up(L, 128)
    bp = torch.zeros(H, L, Lkp); bp[:, :, :L] = r["bias"]
    bT = torch.zeros(H, L, Lqp); bT[:, :, :L] = r["bias"].transpose(1, 2)
    qd, kd, vd, dod = (r[n].reshape(B * L, H * 64).to(dev) for n in ("q", "k", "v", "do"))
    od, lse = torch.empty_like(qd), torch.empty(B * H * L, device=dev)
    v3 = lambda t: K.view3(t, B, L)
    K.attn_fwd(v3(qd), v3(kd), v3(vd), B, B, H, L, L, r["scale"], v3(od), lse, bias=bp.to(dev))
    dq, dk, dv, delta = torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(qd), torch.empty_like(lse)
    args = (v3(qd), v3(kd), v3(vd), v3(od), v3(dod), B, B, H, L, L, r["scale"], lse, delta, v3(dq), v3(dk), v3(dv))
    kw = dict(dS=torch.zeros(B, H, L, Lkp, device=dev, dtype=BF16), bias=bp.to(dev), biasT=bT.to(dev))
    assert K.attn_bwd(*args, ask_form=True, **kw) == 3
    del exact_workspace[:]
    K.attn_bwd(*args, **kw)
    all_ok(*(g for _, g, _ in exact_workspace))
    assert len(exact_workspace) == 1 and exact_workspace[0][2] == B * H * ceil_div(L, 128) * 8192
    assert max(relerr(dq.view(B, L, -1), r["dq"]), relerr(dk.view(B, L, -1), r["dk"]), relerr(dv.view(B, L, -1), r["dv"])) < 1.5e-2
    # relpos_bias_bwd: slices * H * N * ld
    idx = relpos_index(4)
    N, Hh, Bb, ld = 17, 3, 2, 64
    T = int(idx.max()) + 1
    dS = bf(rnd(Bb, Hh, N, ld, seed=6)); dS[..., N:] = 0
    dtab = torch.ones(T, Hh, device=dev)
    del exact_workspace[:]
    K.relpos_bias_bwd(dS.to(dev), idx.to(dev), dtab)
    all_ok(*(g for _, g, _ in exact_workspace))
    assert len(exact_workspace) == 1 and exact_workspace[0][2] == Hh * N * ld
    ref = torch.ones(T, Hh, dtype=torch.float64).index_add_(0, idx.reshape(-1), dS[..., :N].double().sum(0).permute(1, 2, 0).reshape(-1, Hh))
    assert relerr(dtab, ref) < 1e-5
    # embed_bwd / embed_bwd_pid: min(L, R) * D
    V, P, R, L, D = 7, 11, 96, 8, 132
    gen = torch.Generator().manual_seed(3)
    ids, pids, gr = torch.randint(0, V, (R // L, L), generator=gen), torch.randint(0, P, (R // L, L), generator=gen), rnd(R, D, seed=4)
    for pid in (False, True):
        dword, dpos, dtyp = torch.zeros(V, D, device=dev), torch.zeros(P, D, device=dev), torch.zeros(2, D, device=dev)
        del exact_workspace[:]
        if pid:
            K.embed_bwd_pid(ids.to(dev), pids.to(dev), gr.to(dev), dword, dpos, dtyp)
        else:
            K.embed_bwd(ids.to(dev), gr.to(dev), dword, dpos, dtyp)
        all_ok(*(g for _, g, _ in exact_workspace))
        assert len(exact_workspace) == 1 and exact_workspace[0][2] == L * D
        pp = pids.reshape(-1) if pid else torch.arange(R) % L
        assert relerr(dword, torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.reshape(-1), gr.double())) < 1e-5
        assert relerr(dpos, torch.zeros(P, D, dtype=torch.float64).index_add_(0, pp, gr.double())) < 1e-5
        assert relerr(dtyp[0], gr.double().sum(0)) < 1e-5 and float(dtyp[1].abs().max()) == 0.0


def test_gradient_norm_partials_of_the_optimizer():
    """optim.py sizes the partial sums of x2_grad_norm as sum ceil(n / 16384) floats: a guarded buffer of exactly that size in their place"""
    optim = importlib.import_module("x2-vlm_amd.optim")
    sizes = [1, 16384, 16385, 40000]
    params = [torch.nn.Parameter(rnd(n, seed=n).to(dev)) for n in sizes]
    for p in params:
        p.grad = rnd(p.numel(), seed=p.numel() + 1).to(dev)
    params.append(torch.nn.Parameter(torch.zeros(5, device=dev)))          # no gradient
    opt = optim.FusedAdamW(params, lr=1e-4)
    opt._tables()
    rec, nblk, slots, partial, turn = opt._static
    assert nblk == sum(ceil_div(n, 16384) for n in sizes + [5]) and partial.numel() == nblk
    part, gP = guarded((nblk,), F32, tail=nblk, name="grad-norm partials")
    opt._static = (rec, nblk, slots, part, turn)
    out = opt.grad_norm(max_norm=1.0)
    all_ok(gP)
    norm = math.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in params[:-1]))
    assert abs(float(out[0]) - norm) < 1e-5 * norm and abs(float(out[1]) - min(1.0, 1.0 / (norm + 1e-6))) < 1e-5
