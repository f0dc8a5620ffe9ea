"""GPU parity of the captioning-inference kernels (csrc/decode.hip, additive to ABI v14) against float64 on the host.

x2_attn_decode: the new tokens' K/V must land in cache slots hist .. hist + n_new - 1 bit for bit, every other slot of a canary-filled cache
must be untouched, and the outputs must be within 1.5e-2 of the reference's max-abs - the bound test_captioning_kernels_gpu.py applies to the
2-D masked attention forward (the same arithmetic on the same bf16 operands; this kernel keeps the probabilities in fp32, so it sits well
inside it: measured worst 3.7e-3).  x2_beam_gather: bit-exact against index_select, nothing written beyond hist, src == dst refused.
x2_logprob_topk: on logits with spacing >= 1e-3 (no ties in float64) the ids must match exactly and the values to 1e-5; a penalised
log-score is -10000 plus an fp32 value, whose spacing at that magnitude is 9.8e-4, so those entries are held to 1e-3; one constructed tie
pins lowest-column-first."""
import importlib

import pytest
import torch

from kernel_helpers import K, rnd  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
dev = "cuda"
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def D():
    return importlib.import_module("x2-vlm_amd.decode")


def ref_decode(qkv, cache, S, H, n_new, hist, scale):
    """float64: queries of the step over [cached positions < hist ; the step's own K/V], causal by absolute position."""
    Hd = 64 * H
    x = qkv.double().view(S, n_new, 3, H, 64)
    q, kn, vn = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)          # [S, H, n, 64]
    old = cache[:, :hist].double().view(S, hist, 2, H, 64)
    k = torch.cat([old[:, :, 0].transpose(1, 2), kn], 2)
    v = torch.cat([old[:, :, 1].transpose(1, 2), vn], 2)
    s = q @ k.transpose(-1, -2) * scale
    j, c = torch.arange(n_new).view(n_new, 1), torch.arange(hist + n_new).view(1, -1)
    s = s.masked_fill(c > hist + j, float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(S * n_new, Hd)


WORST = {"attn": 0.0}


def run_decode(K, H, S, Lmax, combos, seed):
    Hd = 64 * H
    base = rnd(S, Lmax, 2 * Hd, seed=seed).to(BF16)                       # history and canary at once: every slot holds known bits
    qkv_all = rnd(S, 16, 3 * Hd, seed=seed + 1).to(BF16)
    base_d = base.to(dev)
    scale = 64 ** -0.5
    for n_new, hist in combos:
        qkv = qkv_all[:, :n_new].reshape(S * n_new, 3 * Hd).contiguous()
        cache = base_d.clone()
        out = K.attn_decode(qkv.to(dev), cache, S, H, n_new, hist, scale)
        want_cache = base_d.clone()
        want_cache[:, hist:hist + n_new] = qkv.view(S, n_new, 3 * Hd)[:, :, Hd:].to(dev)
        assert torch.equal(cache.view(torch.int16), want_cache.view(torch.int16)), (H, S, n_new, hist, "cache slots")
        want = ref_decode(qkv, base, S, H, n_new, hist, scale)
        err = float((out.cpu().double() - want).abs().max() / want.abs().max())
        WORST["attn"] = max(WORST["attn"], err)
        assert err < 1.5e-2, (H, S, n_new, hist, err)


@pytest.mark.parametrize("S", [1, 3, 9, 48])
@pytest.mark.parametrize("H", [2, 12, 16])
def test_attn_decode_against_float64(K, H, S):
    combos = [(n, h) for n in (1, 2, 4, 16) for h in (0, 1, 3, 62, 63, 64, 65, 128 - n)]
    run_decode(K, H, S, 128, combos, seed=100 * H + S)
    run_decode(K, H, S, 40, [(1, 39), (2, 38), (4, 36), (16, 24)], seed=100 * H + S + 50)       # a smaller cache, filled to its last slot
    print("attn_decode H=%d S=%d worst relerr so far %.2e" % (H, S, WORST["attn"]))


def test_attn_decode_steps_compose(K):
    """A prompt step followed by two-token steps, each overwriting the previous [MASK] slot, equals one pass over the final tokens."""
    H, S, Lmax = 2, 3, 16
    Hd, scale = 64 * H, 64 ** -0.5
    toks = rnd(S, 8, 3 * Hd, seed=7).to(BF16)                              # projections of the real tokens at positions 0 .. 7
    masks = rnd(S, 8, 3 * Hd, seed=8).to(BF16)                             # those of the [MASK] fed at each position
    cache = torch.full((S, Lmax, 2 * Hd), 7.0, dtype=BF16, device=dev)
    step = torch.cat([toks[:, :3], masks[:, 3:4]], 1).reshape(S * 4, 3 * Hd).contiguous()
    K.attn_decode(step.to(dev), cache, S, H, 4, 0, scale)
    for pos in range(3, 7):                                                 # feed [token at pos, [MASK] at pos + 1]
        step = torch.cat([toks[:, pos:pos + 1], masks[:, pos + 1:pos + 2]], 1).reshape(S * 2, 3 * Hd).contiguous()
        out = K.attn_decode(step.to(dev), cache, S, H, 2, pos, scale)
    final = torch.cat([toks[:, :7], masks[:, 7:8]], 1).reshape(S * 8, 3 * Hd).contiguous()
    whole = K.attn_decode(final.to(dev), torch.zeros_like(cache), S, H, 8, 0, scale)
    assert torch.equal(out.view(S, 2, Hd), whole.view(S, 8, Hd)[:, 6:])
    assert torch.equal(cache[:, :8, :].cpu(), final.view(S, 8, 3 * Hd)[:, :, Hd:])


def test_attn_decode_refuses_what_it_does_not_do(K):
    H, S = 2, 1
    cache = torch.zeros(S, 128, 256, dtype=BF16, device=dev)
    qkv = lambda n: torch.zeros(S * n, 384, dtype=BF16, device=dev)
    with pytest.raises(Exception, match="n_new"):
        K.attn_decode(qkv(17), cache, S, H, 17, 0, 0.125)
    with pytest.raises(Exception, match="exceeds Lmax"):
        K.attn_decode(qkv(2), cache, S, H, 2, 127, 0.125)
    with pytest.raises(Exception, match="multiple of 8"):
        K.attn_decode(qkv(1), torch.zeros(S, 36, 256, dtype=BF16, device=dev), S, H, 1, 0, 0.125)
    with pytest.raises(Exception, match="Lmax"):
        K.attn_decode(qkv(1), torch.zeros(S, 136, 256, dtype=BF16, device=dev), S, H, 1, 0, 0.125)


@pytest.mark.parametrize("hist", [1, 64, 127])
@pytest.mark.parametrize("layers", [1, 4])
def test_beam_gather(K, layers, hist):
    S, Lmax, W = 9, 128, 256
    src = rnd(layers, S, Lmax, W, seed=layers + hist).to(BF16).to(dev)
    parents = {"identity": torch.arange(S), "permutation": torch.randperm(S, generator=torch.Generator().manual_seed(hist)),
               "duplicated": torch.arange(S) // 3, "first_expand": torch.arange(S) // 3 * 3}
    for kind, parent in parents.items():
        dst = torch.full_like(src, -3.0)
        K.beam_gather(src, dst, parent.to(torch.int32).to(dev), hist)
        want = torch.full_like(src, -3.0)
        want[:, :, :hist] = src.index_select(1, parent.to(dev))[:, :, :hist]
        assert torch.equal(dst.view(torch.int16), want.view(torch.int16)), kind
    with pytest.raises(Exception, match="src == dst"):
        K.beam_gather(src, src, parents["identity"].to(torch.int32).to(dev), hist)


_LOGITS = {}


def spaced_logits(V, ldv, rows):
    """rows of a seeded permutation of V values 2^-9 = 1.95e-3 apart (exact in fp32 up to |x| = 30), NaN in the padding columns"""
    key = (V, ldv, rows)
    if key not in _LOGITS:
        g = torch.Generator().manual_seed(V + rows)
        z = torch.full((rows, ldv), float("nan"))
        step = 2.0 ** -9                                                    # 1.95e-3, exact in fp32
        for r in range(rows):
            z[r, :V] = (torch.randperm(V, generator=g).float() - V // 2) * step
        _LOGITS[key] = z
    return _LOGITS[key]


def topk_ref(scores, k):
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]
    return torch.gather(scores, 1, order), order


@pytest.mark.parametrize("rows", [1, 9, 48])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("V,ldv", [(64, 64), (512, 512), (1000, 1024), (30522, 30528)])
def test_logprob_topk_against_float64(K, D, V, ldv, k, rows):
    z = spaced_logits(V, ldv, rows)
    zd = z.to(dev)
    eos = V - 3
    g = torch.Generator().manual_seed(V + k + rows)
    top = z[:, :V].argmax(1)
    modes = {"empty": (None, 0, 3), "short": ("random", 2, 3), "present": ("random", 9, 3), "argmax": ("argmax", 9, 3), "bigram": ("random", 9, 2)}
    for mode, (kind, seq_len, n) in modes.items():
        seq = torch.randint(0, V, (rows, 12), generator=g, dtype=torch.int32)
        if kind is not None and seq_len >= n:
            seq[:, seq_len - (n - 1):seq_len] = seq[:, 1:n]                # the tail repeats ids 1 .. n-1: id n is banned
            if kind == "argmax":
                seq[:, n] = top.to(torch.int32)
            if rows > 1:
                seq[1, 0:3] = seq[1, 3]
                seq[1, seq_len - 3:seq_len] = seq[1, 3]                    # a a a at the tail: overlapping repeat
        seqs = [seq[r, :seq_len].tolist() for r in range(rows)]
        for forbid in (False, True):
            vals, ids, logs = K.logprob_topk(zd, V, k, seq=None if kind is None else seq.to(dev), seq_len=seq_len, ngram=n if kind else 0,
                                             eos_id=eos, forbid_eos=forbid, want_logs=True)
            want = D.log_scores_reference(z[:, :V], seqs if kind else None, n, eos, forbid)
            wv, wi = topk_ref(want, k)
            assert torch.equal(ids.cpu().long(), wi), (mode, forbid)
            assert float((vals.cpu().double() - wv).abs().max()) <= 1e-5, (mode, forbid)
            pen = want < -5000.0
            got = logs.cpu().double()
            assert torch.equal(got < -5000.0, pen), (mode, forbid)
            assert float((got - want)[~pen].abs().max()) <= 1e-5
            if bool(pen.any()):
                assert float((got - want)[pen].abs().max()) <= 1e-3
            if forbid:
                assert bool((got[:, eos] == -10000.0).all())
            if mode == "argmax":
                assert not bool((ids.cpu().long() == top.view(-1, 1)).any())
            if mode == "short":
                assert not bool(pen.any()) or forbid


def test_logprob_topk_ties_take_the_lowest_column(K):
    V = 512
    z = spaced_logits(V, V, 1).clone()
    z[0, [300, 44, 45]] = 50.0                                              # 44 and 300 fall to the same thread (256 apart), 45 to its neighbour
    z[0, [17, 500]] = 40.0
    vals, ids, _ = K.logprob_topk(z.to(dev), V, 8)
    assert ids[0, :5].tolist() == [44, 45, 300, 17, 500]
    assert float(vals[0, 0]) == float(vals[0, 2]) and float(vals[0, 3]) == float(vals[0, 4])
    flat = torch.zeros(2, 64)                                               # every column equal: columns 0 .. K-1 in order
    vals, ids, _ = K.logprob_topk(flat.to(dev), 64, 8)
    assert ids.tolist() == [list(range(8))] * 2


def test_logprob_topk_refuses_what_it_does_not_do(K):
    z = torch.zeros(2, 64, device=dev)
    with pytest.raises(Exception, match="K=9"):
        K.logprob_topk(z, 64, 9)
    with pytest.raises(Exception, match="eos_id"):
        K.logprob_topk(z, 64, 3, eos_id=64)
    with pytest.raises(Exception, match="seq_len"):
        K.logprob_topk(z, 64, 3, seq=torch.zeros(2, 4, dtype=torch.int32, device=dev), seq_len=5, ngram=3)
