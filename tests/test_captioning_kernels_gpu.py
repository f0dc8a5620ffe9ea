"""GPU parity of the captioning fine-tune's kernels (additive to ABI v14) against float64 restatements on the same bf16-rounded inputs:
2-D masked text self-attention (x2_attn_fwd_mask2d / _bwd_mask2d) with tril, FG-free and random masks, dropout off and on; the 2-D
additive-mask builder; the embedding with explicit position ids; the label-smoothed, weighted fused MLM loss (x2_mlm_ls_fwd / x2_ls_combine /
x2_mlm_ls_bwd).

Tolerances (relative to each tensor's max-abs): bf16 attention outputs and gradients 1.5e-2 (P and dS are rounded to bf16 before the second
MFMA, as in test_kernels_gpu.py); fp32 embedding sums 1e-6; the smoothed loss 1e-6 relative [measured worst 3.6e-8] - tight enough to see the z_ign term, whose ignored column carries a large bias
here; its bf16 logit gradient 6e-3 of max-abs [3.3e-3], plus two checks the smoothing mass dominates: the sum of a row's gradient over the
columns that are neither the label nor the ignored id, 1e-2 of ls x the row scale, and the ignored column element-wise."""
import pytest
import torch

from kernel_helpers import K, relerr, rnd  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu
dev = "cuda"


def tril_mask(B, L):
    return torch.tril(torch.ones(L, L, dtype=torch.long)).expand(B, L, L).contiguous()


def fg_free_mask(B, L, seed):
    """tril, then every [MASK] slot's column zeroed except its own diagonal entry (captioning collate, apply_FG_free)."""
    g = torch.Generator().manual_seed(seed)
    m = tril_mask(B, L).clone()
    for b in range(B):
        n = int(torch.randint(1, max(2, L // 6), (1,), generator=g))
        for p in sorted(torch.randperm(L - 1, generator=g)[:n].tolist()):
            m[b, :, p] = 0
            m[b, p, p] = 1
    return m


def random_mask(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    m = (torch.rand(B, L, L, generator=g) < 0.6).long()
    m[:, torch.arange(L), torch.arange(L)] = 1
    return m


def ref_attention(q, k, v, do, m, B, H, L, scale, keep=None):
    """float64: softmax(q k^T * scale + (1 - m) * -10000) (x keep) v and its gradients; q/k/v/do [B, L, H*64]."""
    def heads(t):
        return t.double().view(B, L, H, 64).permute(0, 2, 1, 3).clone().requires_grad_(True)
    qh, kh, vh = heads(q), heads(k), heads(v)
    s = qh @ kh.transpose(-1, -2) * scale + ((1.0 - m.double()) * -10000.0).unsqueeze(1)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep
    o = p @ vh
    o.backward(do.double().view(B, L, H, 64).permute(0, 2, 1, 3))
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B, L, H * 64)
    return back(o.detach()), back(qh.grad), back(kh.grad), back(vh.grad)


def run_mask2d(K, B, H, L, m, drop_p=0.0, seed=0):
    D = H * 64
    q, k, v, do = (rnd(B * L, D, seed=seed + i).to(torch.bfloat16) for i in range(4))
    atts = m.to(dev)
    mask2d = K.additive_mask2d(atts, -10000.0)
    lp = K.round_up(L, 64)
    assert mask2d.shape == (B, L, lp)
    want_mask = torch.zeros(B, L, lp, dtype=torch.float64)
    want_mask[..., :L] = (1.0 - m.double()) * -10000.0
    assert float((mask2d.cpu().double() - want_mask).abs().max()) == 0.0
    drop = K.dropout_spec(drop_p, 1234 + seed, 7)
    keep = None
    if drop_p > 0:
        idx = ((torch.arange(B).view(B, 1, 1, 1) * H + torch.arange(H).view(1, H, 1, 1)) * L + torch.arange(L).view(1, 1, L, 1)) * lp + \
            torch.arange(L).view(1, 1, 1, L)
        keep = K.dropout_keep(drop, idx).double()
    qd, kd, vd, dod = (t.to(dev) for t in (q, k, v, do))
    od = torch.empty(B * L, D, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(B * H * L, device=dev)
    delta = torch.empty(B * H * L, device=dev)
    dq, dk, dv = (torch.empty(B * L, D, device=dev, dtype=torch.bfloat16) for _ in range(3))
    scale = 64 ** -0.5
    K.attn_fwd_mask2d(K.view3(qd, B, L), K.view3(kd, B, L), K.view3(vd, B, L), B, H, L, scale, K.view3(od, B, L), lse, mask2d, drop=drop)
    K.attn_bwd_mask2d(K.view3(qd, B, L), K.view3(kd, B, L), K.view3(vd, B, L), K.view3(od, B, L), K.view3(dod, B, L), B, H, L, scale, lse, delta,
                      K.view3(dq, B, L), K.view3(dk, B, L), K.view3(dv, B, L), mask2d, drop=drop)
    want = ref_attention(q.view(B, L, D), k.view(B, L, D), v.view(B, L, D), do.view(B, L, D), m, B, H, L, scale, keep)
    got = [t.view(B, L, D) for t in (od, dq, dk, dv)]
    return [relerr(g_, w_) for g_, w_ in zip(got, want)], got


@pytest.mark.parametrize("L", [30, 58, 64, 100])
@pytest.mark.parametrize("H", [12, 16])
def test_attention_mask2d_against_float64(K, L, H):
    B = 3
    worst = 0.0
    for kind, m in (("tril", tril_mask(B, L)), ("fg_free", fg_free_mask(B, L, seed=L + H)), ("random", random_mask(B, L, seed=L * H))):
        for p in (0.0, 0.1):
            errs, _ = run_mask2d(K, B, H, L, m, drop_p=p, seed=L + H)
            worst = max(worst, max(errs))
            assert max(errs) < 1.5e-2, (kind, p, errs)
    print("attention mask2d L=%d H=%d worst relerr %.2e" % (L, H, worst))


def test_attention_mask2d_is_deterministic_and_mask_matters(K):
    B, H, L = 2, 12, 58
    m = fg_free_mask(B, L, seed=3)
    _, a = run_mask2d(K, B, H, L, m, drop_p=0.1, seed=5)
    _, b = run_mask2d(K, B, H, L, m, drop_p=0.1, seed=5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    _, c = run_mask2d(K, B, H, L, tril_mask(B, L), drop_p=0.1, seed=5)
    assert not torch.equal(a[0], c[0])


def test_attention_mask2d_rejects_what_it_does_not_do(K):
    B, H, L = 1, 12, 130
    x = torch.zeros(B * L, H * 64, device=dev, dtype=torch.bfloat16)
    mask2d = torch.zeros(B, L, 192, device=dev)
    lse = torch.empty(B * H * L, device=dev)
    with pytest.raises(Exception, match="Lq == Lk <= 128"):
        K.attn_fwd_mask2d(K.view3(x, B, L), K.view3(x, B, L), K.view3(x, B, L), B, H, L, 0.125, K.view3(x, B, L), lse, mask2d)


def test_embedding_with_position_ids(K):
    B, L, D, V, P = 4, 58, 768, 300, 80
    g_ = torch.Generator().manual_seed(11)
    ids = torch.randint(0, V, (B, L), generator=g_)
    ids[:, 0] = 101
    pids = torch.empty(B, L, dtype=torch.long)
    for b in range(B):                       # FG-free: repeated positions, sequences sharing ids
        seq, i = [], 0
        while len(seq) < L:
            if b % 2 == 0 and torch.rand(1, generator=g_).item() < 0.3 and len(seq) < L - 1:
                seq += [i, i]
            else:
                seq.append(i)
            i += 1
        pids[b] = torch.tensor(seq[:L])
    word, pos, typ = rnd(V, D, seed=12), rnd(P, D, seed=13), rnd(D, seed=14)
    gout = rnd(B * L, D, seed=15)
    idd, pidd = ids.to(dev), pids.to(dev)
    out = K.embed_fwd_pid(idd, pidd, word.to(dev), pos.to(dev), typ.to(dev))
    want = word.double()[ids.view(-1)] + pos.double()[pids.view(-1)] + typ.double()
    assert relerr(out, want) < 1e-6
    dword, dpos, dtyp = torch.zeros(V, D, device=dev), torch.zeros(P, D, device=dev), torch.zeros(D, device=dev)
    K.embed_bwd_pid(idd, pidd, gout.to(dev), dword, dpos, dtyp)
    rw = torch.zeros(V, D, dtype=torch.float64).index_add_(0, ids.view(-1), gout.double())
    rp = torch.zeros(P, D, dtype=torch.float64).index_add_(0, pids.view(-1), gout.double())
    assert relerr(dword, rw) < 1e-6 and relerr(dpos, rp) < 1e-6 and relerr(dtyp, gout.double().sum(0)) < 1e-6
    # fixed-order sums: a second run gives the same bits
    dword2, dpos2, dtyp2 = torch.zeros_like(dword), torch.zeros_like(dpos), torch.zeros_like(dtyp)
    K.embed_bwd_pid(idd, pidd, gout.to(dev), dword2, dpos2, dtyp2)
    assert torch.equal(dword, dword2) and torch.equal(dpos, dpos2) and torch.equal(dtyp, dtyp2)
    # with pids = r % L it is the plain embedding
    plain = torch.arange(L).expand(B, L).contiguous().to(dev)
    assert torch.equal(K.embed_fwd_pid(idd, plain, word.to(dev), pos.to(dev), typ.to(dev)), K.embed_fwd(idd, word.to(dev), pos.to(dev), typ.to(dev)))


def ref_smoothed(z, labels, w, V, ignore, ls):
    """float64 LabelSmoothingLoss + loss_mask_and_normalize of the captioning fine-tune, and d loss / d z."""
    z = z.clone().requires_grad_(True)
    q = torch.full((z.shape[0], V), ls / (V - 2), dtype=torch.float64)
    q[:, ignore] = 0
    q.scatter_(1, labels.view(-1, 1), 1.0 - ls)
    q[labels == ignore] = 0
    kl = torch.nn.functional.kl_div(torch.log_softmax(z, -1), q, reduction="none").sum(-1)
    loss = (kl * w.double() / (w.double().sum() + 1e-5)).sum()
    loss.backward()
    return loss.detach(), z.grad


@pytest.mark.parametrize("V,Hd,ignore", [(30522, 1024, 101), (250, 128, 2)])
def test_smoothed_mlm_loss(K, V, Hd, ignore):
    R, ls = 48, 0.1
    Vp = K.round_up(V, 64)
    x = rnd(R, Hd, seed=31).to(torch.bfloat16)
    E = torch.zeros(Vp, Hd)
    E[:V] = rnd(V, Hd, seed=32, scale=3.0 * Hd ** -0.5)
    E = E.to(torch.bfloat16)
    bias = torch.zeros(Vp)
    bias[:V] = rnd(V, seed=33)
    bias[ignore] = 20.0                           # z_ign large: its term in the loss is visible at V = 30522
    g_ = torch.Generator().manual_seed(34)
    labels = torch.randint(0, V, (R,), generator=g_)
    labels[::7] = ignore                          # padded slots: PAD_mask = the ignored id, weight 0
    labels[1] = V - 1
    w = torch.ones(R)
    w[::7] = 0.0
    w[3] = 0.0                                    # a real label with weight 0
    xd, Ed, bd, ld, wd = x.to(dev), E.to(dev), bias.to(dev), labels.to(dev), w.to(dev)
    stat, lse = K.mlm_ls_fwd(xd, Ed, bd, ld, wd, V, ignore, ls)
    z = x.double() @ E.double().t()[:, :V] + bias[:V].double()
    want, dz = ref_smoothed(z, labels, w, V, ignore, ls)
    assert float((lse.cpu().double() - torch.logsumexp(z, -1)).abs().max()) < 1e-4
    err = abs(float(stat[0]) - float(want)) / max(1.0, abs(float(want)))
    assert err < 1e-6, (float(stat[0]), float(want))
    assert float(stat[1]) == float(w.sum())
    g = torch.tensor([0.7], device=dev)
    dl = K.mlm_ls_bwd(xd, Ed, bd, ld, wd, lse, g, stat, V, ignore, ls)
    assert relerr(dl[:, :V], dz * 0.7) < 6e-3
    assert float(dl[:, V:].float().abs().max()) == 0.0 if Vp > V else True
    dead = (labels == ignore) | (w == 0)
    assert float(dl[dead.to(dev)].float().abs().max()) == 0.0
    # the smoothing mass: sum over off-label, non-ignored columns = sc * (sum(q) * sum p - ls); q[c] = 0 off the label would miss ls * sc
    got, ref = dl[:, :V].double().cpu(), dz * 0.7
    live = ~dead
    off = torch.ones(R, V, dtype=torch.bool)
    off[torch.arange(R), labels] = False
    off[:, ignore] = False
    sc = 0.7 * w / (w.sum() + 1e-5)
    s_got, s_ref = (got * off).sum(1), (ref * off).sum(1)
    assert bool(((s_got - s_ref).abs()[live] <= 1e-2 * ls * sc[live]).all())
    # the ignored column: q[ignore] = 0, so dl = sum(q) p sc there (q = s would shift it by s * sc)
    s_ = ls / (V - 2)
    e_ign = (got[:, ignore] - ref[:, ignore]).abs()
    assert bool((e_ign[live] <= 2 ** -8 * ref[:, ignore].abs()[live] + 1e-3 * s_ * sc[live]).all())
    print("smoothed loss V=%d rel err %.2e, dl relerr %.2e" % (V, err, relerr(dl[:, :V], dz * 0.7)))
