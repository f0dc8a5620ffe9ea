"""GPU parity of the VQA answer-ranking kernels (csrc/vqa.hip, additive to ABI v14) against float64 on the host with the same tie rule
(larger value first, lower index first among equal values: cases_vqa.first_stage / second_stage).

x2_answer_topk: logits are a seeded permutation of a 2^-9 grid plus a row offset, so distinct tokens' logits are more than 1e-3 apart
(asserted) and only candidates sharing a first token tie - exactly; the ids must then match exactly and the values to 1e-5, the bound
test_decode_kernels_gpu.py applies to x2_logprob_topk's values (the same arithmetic).  The padding columns hold NaN (never read), canaries
after both outputs stay intact, every limit violation is an error without a launch.  Beyond the issue's shapes: Na = 8200, past the 8192
log-probabilities the kernel keeps in LDS (the rest are recomputed every round).
x2_vqa_candidates: bit-exact (as int32 bit patterns for the mask) against the torch construction of the reference: index_select,
masked_fill, tile and (1 - tril x atts) * -10000 padded to 64 columns; rows that are all padding after the start token included.
x2_vqa_rerank: scores within (La) * 2^-24 * sum|terms| of float64 - sequential fp32 summation of La terms (Higham, gamma_n <= n u for the
running sums, u = 2^-24) - with inputs placed so that float64 scores differ by more than 100 times that (asserted), but for one pair of
slots with identical bits per question (lowest slot first); order exact, probabilities within twice the score bound relative plus 1e-7.
mlm_ce_rows: lse bit-equal to mlm_ce_fwd's, loss_row 0 where the label is -100, its mean over the counted rows mlm_ce_fwd's loss, and
lse - z[label] of the same bf16 operands in float64 within the fp32 accumulation bound of the Hd-term dot products."""
import numpy as np
import pytest
import torch

from cases_vqa import first_stage, second_stage
from kernel_helpers import K  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
dev = "cuda"
F32, I32, I64 = torch.float32, torch.int32, torch.int64
CANARY = 8


_LOGITS = {}


def spaced_logits(V, ldv, rows):
    """rows of a seeded permutation of V values 2^-9 apart plus a row offset (exact in fp32: |x| < 64), NaN in the padding columns"""
    key = (V, ldv, rows)
    if key not in _LOGITS:
        g = torch.Generator().manual_seed(7 * V + rows)
        z = torch.full((rows, ldv), float("nan"))
        for r in range(rows):
            z[r, :V] = (torch.randperm(V, generator=g).float() - V // 2) * 2.0 ** -9 + 0.25 * r
        srt = torch.sort(z[:, :V].double(), 1).values
        assert float((srt[:, 1:] - srt[:, :-1]).min()) > 1e-3                  # distinct tokens never come closer than this
        _LOGITS[key] = (z, z.to(dev), torch.log_softmax(z[:, :V].double(), -1))
    return _LOGITS[key]


def first_tokens(kind, Na, V, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "distinct":
        return torch.randperm(V, generator=g)[:Na].to(I32)
    if kind == "equal":
        return torch.full((Na,), int(torch.randint(0, V, (1,), generator=g)), dtype=I32)
    pool = torch.randperm(V, generator=g)[:max(1, Na // 3)]
    return pool[torch.randint(0, pool.numel(), (Na,), generator=g)].to(I32)


def run_answer_topk(K, zd, V, ft_d, k):
    """the raw entry point on canary-padded outputs -> (vals [B, k], ids [B, k]) on the host"""
    B = zd.shape[0]
    vals = torch.full((B * k + CANARY,), -777.0, device=dev, dtype=F32)
    ids = torch.full((B * k + CANARY,), -777, device=dev, dtype=I32)
    K.call("x2_answer_topk", K.ptr(zd), zd.stride(0), V, B, K.ptr(ft_d), ft_d.numel(), k, K.ptr(vals), K.ptr(ids))
    vals, ids = vals.cpu(), ids.cpu()
    assert bool((vals[B * k:] == -777.0).all()) and bool((ids[B * k:] == -777).all())
    return vals[:B * k].view(B, k), ids[:B * k].view(B, k)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("V,ldv", [(512, 512), (500, 512), (30522, 30528)])
def test_answer_topk_against_float64(K, V, ldv, B):
    z, zd, logsm = spaced_logits(V, ldv, B)
    worst = 0.0
    for Na in (1, 7, 64, 65, 257, 3128):
        for kind in ("distinct", "third", "equal"):
            if kind == "distinct" and Na > V:
                continue
            ft = first_tokens(kind, Na, V, Na + len(kind))
            ft_d = ft.to(dev)
            logp = logsm.index_select(1, ft.long()).numpy()
            for k in sorted({kk for kk in (1, 3, 64, 128, 256, Na) if kk <= min(Na, 256)}):
                vals, ids = run_answer_topk(K, zd, V, ft_d, k)
                wv, wi = first_stage(logp, k)
                assert np.array_equal(ids.numpy().astype(np.int64), wi), (Na, kind, k)
                err = float(np.abs(vals.numpy().astype(np.float64) - wv).max())
                worst = max(worst, err)
                assert err <= 1e-5, (Na, kind, k, err)
                if kind == "equal":
                    assert ids.tolist() == [list(range(k))] * B
    print("x2_answer_topk V=%d B=%d: worst |value - float64| %.3e (bound 1e-5)" % (V, B, worst))


def test_answer_topk_wrapper_and_candidates_past_the_lds_cache(K):
    V, B, Na = 30522, 2, 8200
    z, zd, logsm = spaced_logits(V, 30528, B)
    ft = first_tokens("third", Na, V, 5)
    # the best tokens of both rows sit at the very end of the list, twice each: found past the cached prefix, lowest index first
    top = logsm.argmax(1)
    ft[Na - 4:] = torch.stack([top, top]).reshape(-1).to(I32)
    for k in (3, 256):
        vals, ids = K.answer_topk(zd, V, ft.to(dev), k)
        assert vals.shape == (B, k) and ids.shape == (B, k) and vals.dtype == F32 and ids.dtype == I32
        wv, wi = first_stage(logsm.index_select(1, ft.long()).numpy(), k)
        assert np.array_equal(ids.cpu().numpy().astype(np.int64), wi)
        assert float(np.abs(vals.cpu().numpy().astype(np.float64) - wv).max()) <= 1e-5
    assert sorted(ids[0, :2].tolist()) == sorted(i for i in range(Na - 4, Na) if int(ft[i]) == int(top[0]))


def test_answer_topk_refuses_what_it_does_not_do(K):
    z = torch.zeros(2, 64, device=dev)
    ft = torch.zeros(300, dtype=I32, device=dev)
    for k, n, what in ((0, 300, "k=0"), (301, 300, "k=301"), (257, 300, "k=257"), (8, 7, "k=8")):
        with pytest.raises(Exception, match=what):
            K.answer_topk(z, 64, ft[:n], k)
    with pytest.raises(Exception, match="Na=65537"):
        K.answer_topk(z, 64, torch.zeros(65537, dtype=I32, device=dev), 8)
    with pytest.raises(Exception, match="ldv"):
        K.call("x2_answer_topk", K.ptr(z), 32, 64, 2, K.ptr(ft), 300, 8, K.ptr(z), K.ptr(ft))
    torch.cuda.synchronize()


def candidate_reference(answer_ids, answer_atts, ids, pad):
    """the reference's construction in torch (model_generation.py:581-593 and the decoder's extended mask), on the host"""
    B, k = ids.shape
    La = answer_ids.shape[1]
    flat = ids.reshape(-1).long()
    input_ids = answer_ids.index_select(0, flat)
    atts = answer_atts.index_select(0, flat)
    labels = input_ids.masked_fill(input_ids == pad, -100)[:, 1:]
    kv = (torch.arange(B * k) // k).to(I32)
    ext = torch.tril(torch.ones(La, La, dtype=I64))[None] * atts[:, None, :]
    Lp = (La + 63) // 64 * 64
    mask = torch.zeros(B * k, La, Lp)
    mask[:, :, :La] = (1.0 - ext.to(F32)) * -10000.0
    return input_ids, labels, kv, mask


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("La", [2, 5, 64, 65, 128])
def test_vqa_candidates_bit_exact(K, La, k, B):
    Na = 11
    for pad in (0, 7):
        g = torch.Generator().manual_seed(La * 100 + k * 10 + B + pad)
        answer_ids = torch.randint(8, 500, (Na, La), generator=g)
        lens = torch.randint(2, La + 1, (Na,), generator=g)
        lens[0], lens[3], lens[5] = La, 1, 1                                   # rows 3 and 5: all padding after the start token
        answer_atts = (torch.arange(La)[None] < lens[:, None]).to(I64)
        answer_ids = torch.where(answer_atts == 1, answer_ids, torch.full_like(answer_ids, pad))
        answer_ids[:, 0] = 1
        ids = torch.randint(0, Na, (B, k), generator=g).to(I32)
        ids[0, 0] = 3
        if k > 1:
            ids[B - 1, k - 1], ids[0, 1] = 5, 0
        got = K.vqa_candidates(answer_ids.to(dev), answer_atts.to(dev), ids.to(dev), pad)
        want = candidate_reference(answer_ids, answer_atts, ids, pad)
        for name, a, b in zip(("input_ids", "labels", "kv_idx", "mask2d"), got, want):
            assert a.shape == b.shape and a.dtype == b.dtype, name
            a = a.cpu()
            if name == "mask2d":
                a, b = a.view(I32), b.view(I32)
            assert torch.equal(a, b), (name, pad)
        assert bool((got[1][0] == -100).all())                                # the all-padding row scores no token


def test_vqa_candidates_limits_and_stray_ids(K):
    answer_ids = torch.ones(4, 129, dtype=I64, device=dev)
    ids = torch.zeros(1, 2, dtype=I32, device=dev)
    with pytest.raises(Exception, match="La=129"):
        K.vqa_candidates(answer_ids, answer_ids.clone(), ids, 0)
    with pytest.raises(Exception):
        K.vqa_candidates(answer_ids[:, :1].contiguous(), answer_ids[:, :1].contiguous(), ids, 0)
    # an id outside the list reads nothing: an all-padding row
    a5 = torch.full((4, 5), 9, dtype=I64, device=dev)
    bad = torch.tensor([[1, 4], [-1, 2 ** 31 - 1]], dtype=I32, device=dev)
    input_ids, labels, kv, mask = K.vqa_candidates(a5, torch.ones_like(a5), bad, 0)
    assert input_ids.tolist() == [[9] * 5, [0] * 5, [0] * 5, [0] * 5] and labels[1:].eq(-100).all() and kv.tolist() == [0, 0, 1, 1]
    assert bool((mask[1:, :, :5] == -10000.0).all()) and bool((mask[:, :, 5:] == 0).all())


@pytest.mark.parametrize("T", [1, 2, 7, 127])
@pytest.mark.parametrize("k", [1, 2, 3, 64, 128, 256])
def test_vqa_rerank_against_float64(K, k, T):
    B, u = 2, 2.0 ** -24
    g = torch.Generator().manual_seed(1000 * k + T)
    loss = torch.rand(B * k, T, generator=g) * 2.0
    loss[torch.rand(B * k, T, generator=g) < 0.3] = 0.0                        # ignored positions
    loss[torch.randperm(B * k, generator=g)[:max(1, k // 8)]] = 0.0            # candidates with nothing but the first token
    target = torch.stack([torch.randperm(k, generator=g) for _ in range(B)]).double() * -1.0 - 0.5     # scores one apart, shuffled
    vals = (target + loss.double().sum(1).view(B, k)).to(F32)
    if k >= 2:                                                                 # two slots with identical bits per question
        for b in range(B):
            i, j = sorted(torch.randperm(k, generator=g)[:2].tolist())
            loss[b * k + j] = loss[b * k + i]
            vals[b, j] = vals[b, i]
    ids = torch.stack([torch.randperm(5000, generator=g)[:k] for _ in range(B)]).to(I32)
    want = vals.double() - loss.double().sum(1).view(B, k)
    bound = (T + 1) * u * (vals.double().abs() + loss.double().abs().sum(1).view(B, k))
    srt = torch.sort(want, 1, descending=True).values
    gaps = srt[:, :-1] - srt[:, 1:]
    assert int((gaps == 0).sum()) == (B if k >= 2 else 0) and bool((gaps[gaps > 0] > 100 * bound.max()).all())
    probs, top, scores = (t.cpu() for t in K.vqa_rerank(loss.to(dev), vals.to(dev), ids.to(dev)))
    err = (scores.double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    wp, wi = second_stage(want.numpy(), ids.numpy())
    assert np.array_equal(top.numpy().astype(np.int64), wi)
    perr = np.abs(probs.numpy().astype(np.float64) - wp)
    assert bool((perr <= 2 * float(bound.max()) * wp + 1e-7).all()), float(perr.max())
    assert abs(float(probs.double().sum(1).max()) - 1) <= 1e-5 and bool((probs[:, :-1] >= probs[:, 1:]).all())
    print("x2_vqa_rerank k=%d T=%d: worst score error / bound %.3f, worst |prob - float64| %.3e" % (k, T, float((err / bound).max()), float(perr.max())))


def test_vqa_rerank_limits(K):
    loss = torch.zeros(2 * 257, 3, device=dev)
    vals = torch.zeros(2, 257, device=dev)
    with pytest.raises(Exception, match="k=257"):
        K.vqa_rerank(loss, vals, torch.zeros(2, 257, dtype=I32, device=dev))
    with pytest.raises(Exception, match="128"):
        K.vqa_rerank(torch.zeros(4, 128, device=dev), vals[:, :2].contiguous(), torch.zeros(2, 2, dtype=I32, device=dev))


def test_mlm_ce_rows_is_the_existing_path_per_row(K):
    R, Hd, V, Vp = 37, 128, 500, 512
    g = torch.Generator().manual_seed(3)
    x = torch.randn(R, Hd, generator=g).to(torch.bfloat16)
    E = torch.zeros(Vp, Hd)
    E[:V] = torch.randn(V, Hd, generator=g) * 0.2
    E = E.to(torch.bfloat16)
    bias = torch.zeros(Vp)
    bias[:V] = torch.randn(V, generator=g) * 0.1
    labels = torch.randint(0, V, (R,), generator=g)
    labels[[0, 5, 36]] = -100
    args = (x.to(dev), E.to(dev), bias.to(dev), labels.to(dev), V)
    stat, lse_old = K.mlm_ce_fwd(*args)
    loss_row, lse = K.mlm_ce_rows(*args)
    assert torch.equal(lse, lse_old) and loss_row.shape == (R,) and loss_row.dtype == F32
    keep = labels >= 0
    assert bool((loss_row.cpu()[~keep] == 0).all()) and float(stat[1]) == int(keep.sum())
    assert abs(float(loss_row.double().sum()) / int(keep.sum()) - float(stat[0])) <= 1e-6 * float(stat[0])
    z = x.double() @ E.double().t() + bias.double()
    want = torch.logsumexp(z[:, :V], -1) - torch.gather(z, 1, labels.clamp(min=0).view(-1, 1)).view(-1)
    # fp32 accumulation of Hd products per logit: Hd * 2^-24 * sum |x| |E|, for the label's logit and (at most) for the logsumexp
    bound = 2 * Hd * 2.0 ** -24 * float((x.double().abs() @ E.double().abs().t()).max()) + 1e-5
    err = float((loss_row.cpu().double() - want)[keep].abs().max())
    print("mlm_ce_rows: worst |loss_row - float64| %.3e (bound %.3e)" % (err, bound))
    assert err <= bound
