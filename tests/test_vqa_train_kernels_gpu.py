"""GPU parity of the VQA training step's kernels (csrc/vqa.hip, csrc/gemm.hip epilogue variant 13; additive to ABI v14) against float64 from the
same bf16 operands.  Every output lives in a kernel_helpers.guarded buffer: a write outside the documented extent fails the test.

x2_vqa_train_rows: bit-exact (the mask as int32 bit patterns) against the torch construction of the reference: repeat_interleave of the question
index, masked_fill of the next tokens, (1 - tril x atts) * -10000 padded to 64 columns, weights / B; padding rows behind sum(k) get the last
question, labels -100 and c = 0 whatever weight they carry.
x2_mlm_ce_fwd + x2_seq_loss_combine: loss_seq within T x the bound tests/test_vqa_kernels_gpu.py holds mlm_ce_rows to (fp32 accumulation of the
Hd-term dot products, for the label's logit and for the logsumexp, + 1e-5); total within 1e-6 relative of the float64 weighted sum of the
kernel's own loss_seq plus (S + 1) * 2^-24 * sum |c loss_seq| (sequential fp32 summation, the bound of x2_vqa_rerank's scores).
x2_mlm_seq_bwd: the logit gradient within 6e-3 of its max-abs (tests/test_captioning_kernels_gpu.py's bound for x2_mlm_ls_bwd); exact zeros on
ignored rows, on the rows of c == 0 sequences and in the pad columns; (c / 2, g = 2) and (c, g = 1) give the same bits.
Every kernel gives the same bits twice.

BertLMHeadModel.forward(labels=..., reduction='none') at tiny: .loss equals the per-row values of head_loss_rows added in index order BIT FOR BIT -
the same bf16 rows go through the same transform and the same x2_mlm_ce_fwd launch, x2_seq_loss_combine folds the chunk statistics with
x2_ce_combine's arithmetic, and the kernel adds a row's T values one after the other in fp32, which is what the test does; reduction='mean'
equals sum / count to 1e-6.

Measured on the MI355X (printed by the tests), worst over S in {1, 6, 33}, T in {1, 4, 7} and both label patterns, per (V, Vp, Hd): loss_seq
at most 0.004 of its bound, total at most 0.067 of its bound, the logit gradient 3.1e-3 of max-abs at V <= 512 and 7.5e-4 at V = 30522 (bound
6e-3)."""
import importlib

import pytest
import torch

from cases_vqa_train import VQA_TRAIN_CASES, vqa_train_batch, vqa_train_config
from kernel_helpers import _ALIVE, K, guarded, relerr  # noqa: F401 (fixture)

pytestmark = pytest.mark.gpu
dev = "cuda"
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64
U = 2.0 ** -24


def release():
    """the guarded allocations made so far: nothing in flight reads them any more"""
    torch.cuda.synchronize()
    del _ALIVE[:]


@pytest.fixture(autouse=True)
def _release_allocations():
    yield
    release()


# ----------------------------------------------------------------------------------------------------------------- the row builder

def rows_reference(offs, answer_ids, answer_atts, weights, B, pad):
    """the reference's construction in torch, on the host (model_generation.py:522-548 and the decoder's extended mask)"""
    S, La = answer_ids.shape
    n = int(offs[B])
    k = (offs[1:] - offs[:-1]).long()
    kv = torch.full((S,), B - 1, dtype=I32)
    kv[:n] = torch.repeat_interleave(torch.arange(B), k).to(I32)
    labels = answer_ids.masked_fill(answer_ids == pad, -100)[:, 1:].clone()
    labels[n:] = -100
    ext = torch.tril(torch.ones(La, La, dtype=I64))[None] * answer_atts[:, None, :]
    Lp = (La + 63) // 64 * 64
    mask = torch.zeros(S, La, Lp)
    mask[:, :, :La] = (1.0 - ext.to(F32)) * -10000.0
    c = weights / float(B)
    c[n:] = 0.0
    return kv, labels, mask, c


@pytest.mark.parametrize("La", [2, 5, 64, 65, 128])
@pytest.mark.parametrize("npad", [0, 3])
@pytest.mark.parametrize("k", [[1], [3, 1, 2], [1, 1, 1]], ids=["k1", "k312", "k111"])
def test_vqa_train_rows_bit_exact(K, k, npad, La):
    B, n = len(k), sum(k)
    S = n + npad
    Lp = (La + 63) // 64 * 64
    for pad in (0, 7):
        g = torch.Generator().manual_seed(La * 1000 + n * 10 + npad + pad)
        ids = torch.randint(8, 500, (S, La), generator=g)
        lens = torch.randint(2, La + 1, (S,), generator=g)
        lens[0] = La
        if n > 1:
            lens[1] = 1                                                        # a real row that is all padding after the start token
        atts = (torch.arange(La)[None] < lens[:, None]).to(I64)
        ids = torch.where(atts == 1, ids, torch.full_like(ids, pad))
        ids[:, 0] = 1
        ids[n:], atts[n:] = pad, 0                                             # padding rows: a valid id, attention 0 ...
        weights = torch.randint(1, 11, (S,), generator=g).float() / 10.0       # ... and a weight the kernel must zero
        offs = torch.zeros(B + 1, dtype=I32)
        offs[1:] = torch.cumsum(torch.tensor(k), 0)
        want = rows_reference(offs, ids, atts, weights.clone(), B, pad)
        outs = [guarded((S,), I32, name="kv_idx"), guarded((S, La - 1), I64, name="labels"), guarded((S, La, Lp), F32, name="mask2d"),
                guarded((S,), F32, name="c")]
        args = [t.to(dev) for t in (offs, ids, atts, weights)]
        runs = []
        for _ in range(2):
            K.call("x2_vqa_train_rows", *(K.ptr(t) for t in args), B, S, La, pad, K.ptr(outs[0][0]), K.ptr(outs[1][0]), K.ptr(outs[2][0]), Lp,
                   K.ptr(outs[3][0]))
            for _, guard in outs:
                guard()
            runs.append([v.cpu().clone() for v, _ in outs])
        for name, a, b, w in zip(("kv_idx", "labels", "mask2d", "c"), runs[0], runs[1], want):
            assert a.shape == w.shape and a.dtype == w.dtype, name
            if a.dtype == F32:
                a, b, w = a.view(I32), b.view(I32), w.view(I32)
            assert torch.equal(a, w), (name, pad)
            assert torch.equal(a, b), name
        if npad:
            assert bool((runs[0][1][n:] == -100).all()) and bool((runs[0][3][n:] == 0).all()) and bool((runs[0][0][n:] == B - 1).all())
            assert bool((runs[0][2][n:, :, :La] == -10000.0).all())            # fully masked rows: finite, the softmax stays uniform
    # the wrapper: same values, its own allocations
    got = K.vqa_train_rows(*args, pad)
    for a, w in zip(got, want):
        assert torch.equal(a.cpu(), w)


def test_vqa_train_rows_limits(K):
    ids = torch.ones(4, 129, dtype=I64, device=dev)
    offs = torch.tensor([0, 4], dtype=I32, device=dev)
    w = torch.ones(4, device=dev)
    with pytest.raises(Exception, match="La=129"):
        K.vqa_train_rows(offs, ids, ids.clone(), w, 0)
    with pytest.raises(Exception):                                              # La = 1: no label to write, refused before a launch
        K.vqa_train_rows(offs, ids[:, :1].contiguous(), ids[:, :1].contiguous(), w, 0)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- the per-sequence loss

_OPERANDS = {}


def operands(V, Vp, Hd):
    """(E bf16 [Vp, Hd] with zero pad rows, bias fp32 [Vp] with zero pad, both on the device) - built once per geometry and left unchanged"""
    key = (V, Vp, Hd)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(V + Hd)
        E = torch.zeros(Vp, Hd)
        E[:V] = torch.randn(V, Hd, generator=g) * (0.2 if Hd == 128 else 0.08)
        bias = torch.zeros(Vp)
        bias[:V] = torch.randn(V, generator=g) * 0.1
        _OPERANDS[key] = (E.to(BF16).to(dev), bias.to(dev))
    return _OPERANDS[key]


def sequence_case(S, T, V, Hd, pattern):
    g = torch.Generator().manual_seed(S * 100 + T * 10 + Hd + V)
    R = S * T
    x = torch.randn(R, Hd, generator=g).to(BF16)
    labels = torch.randint(0, V, (S, T), generator=g)
    labels[torch.rand(S, T, generator=g) < 0.25] = -100
    labels[0, 0] = V - 1                                                        # the last valid column, next to the pad columns
    c = torch.randint(1, 9, (S,), generator=g).float() / 8.0                  # multiples of 1/8: halving and doubling are exact
    if pattern == "all_ignored":
        labels[S // 2] = -100                                                   # a sequence with every label ignored (its c stays non-zero)
    if S > 2:
        c[S - 1] = 0.0                                                          # a sequence with weight 0 and real labels
        labels[S - 1, T - 1] = 3
    return x.to(dev), labels.reshape(-1).contiguous().to(dev), c.to(dev)


def run_forward(K, x, E, bias, labels, V, S, T, c):
    R, Vp = x.shape[0], E.shape[0]
    part, g_part = guarded((R * (Vp // 64) * 2,), F32, name="part")
    zlab, g_zlab = guarded((R,), F32, name="zlab")
    lse, g_lse = guarded((R,), F32, name="lse")
    loss_seq, g_seq = guarded((S,), F32, name="loss_seq")
    total, g_total = guarded((1,), F32, name="total")
    K.call("x2_mlm_ce_fwd", K.ptr(x), K.ptr(E), K.ptr(bias), K.ptr(labels), R, Vp, V, x.shape[1], x.stride(0), E.stride(0), K.ptr(part), K.ptr(zlab))
    K.call("x2_seq_loss_combine", K.ptr(part), Vp // 64, K.ptr(zlab), K.ptr(labels), S, T, K.ptr(c), K.ptr(lse), K.ptr(loss_seq),
           K.ptr(total) if c is not None else None)
    for guard in (g_part, g_zlab, g_lse, g_seq) + ((g_total,) if c is not None else ()):
        guard()
    return lse, loss_seq, total if c is not None else None


def run_backward(K, x, E, bias, labels, c, lse, gval, V, T):
    R, Vp = x.shape[0], E.shape[0]
    dl, g_dl = guarded((R, Vp), BF16, name="dl")
    g = torch.tensor([gval], device=dev, dtype=F32)
    K.call("x2_mlm_seq_bwd", K.ptr(x), K.ptr(E), K.ptr(bias), K.ptr(labels), K.ptr(c), K.ptr(lse), K.ptr(g), T, R, Vp, V, x.shape[1], x.stride(0),
           E.stride(0), K.ptr(dl), Vp)
    g_dl()
    return dl


@pytest.mark.parametrize("Hd", [128, 768])
@pytest.mark.parametrize("V,Vp", [(512, 512), (500, 512), (30522, 30528)])
def test_sequence_loss_forward_and_backward_against_float64(K, V, Vp, Hd):
    E, bias = operands(V, Vp, Hd)
    E64, b64 = E.double(), bias.double()
    worst = dict(seq=0.0, total=0.0, dz=0.0)
    for S in (1, 6, 33):
        for T in (1, 4, 7):
            for pattern in ("mixed", "all_ignored"):
                x, labels, c = sequence_case(S, T, V, Hd, pattern)
                R = S * T
                lse, loss_seq, total = run_forward(K, x, E, bias, labels, V, S, T, c)
                lse2, loss_seq2, total2 = run_forward(K, x, E, bias, labels, V, S, T, c)
                assert torch.equal(lse, lse2) and torch.equal(loss_seq, loss_seq2) and torch.equal(total, total2)
                # float64 on the device, from the same bf16 operands
                z = (x.double() @ E64.t() + b64)[:, :V]
                lse64 = torch.logsumexp(z, -1)
                keep = labels >= 0
                row = torch.where(keep, lse64 - torch.gather(z, 1, labels.clamp(min=0).view(-1, 1)).view(-1), torch.zeros_like(lse64))
                want_seq = row.view(S, T).sum(1)
                bound = T * (2 * Hd * U * float((x.double().abs() @ E64.abs().t()).max()) + 1e-5)
                e_seq = float((loss_seq.double() - want_seq).abs().max())
                worst["seq"] = max(worst["seq"], e_seq / bound)
                assert e_seq <= bound, (S, T, pattern, e_seq, bound)
                dead_seq = ~keep.view(S, T).any(1)
                assert bool((loss_seq[dead_seq] == 0).all())                                    # ignored positions add exactly 0
                terms = c.double() * loss_seq.double()
                want_total = float(terms.sum())
                b_total = 1e-6 * abs(want_total) + (S + 1) * U * float(terms.abs().sum())
                e_total = abs(float(total[0]) - want_total)
                worst["total"] = max(worst["total"], e_total / max(b_total, 1e-30))
                assert e_total <= b_total, (S, T, pattern, e_total, b_total)
                # without c: the same loss_seq bits, total untouched
                _, loss_seq3, none = run_forward(K, x, E, bias, labels, V, S, T, None)
                assert none is None and torch.equal(loss_seq3, loss_seq)
                # backward: scalar g with c, against float64
                gval = 0.75
                dl = run_backward(K, x, E, bias, labels, c, lse, gval, V, T)
                assert torch.equal(dl, run_backward(K, x, E, bias, labels, c, lse, gval, V, T))
                sc = (c.double().repeat_interleave(T) * gval * keep.double()).view(-1, 1)
                onehot = torch.zeros_like(z)
                onehot[torch.arange(R, device=dev)[keep], labels[keep]] = 1.0
                want_dz = (torch.softmax(z, -1) - onehot) * sc
                if float(want_dz.abs().max()) > 0:
                    e_dz = relerr(dl[:, :V], want_dz.cpu())
                    worst["dz"] = max(worst["dz"], e_dz)
                    assert e_dz < 6e-3, (S, T, pattern, e_dz)
                bits = dl.view(torch.int16)
                dead_rows = ~keep | (c.repeat_interleave(T) == 0)
                assert bool((bits[dead_rows] == 0).all())                                       # exact (positive) zeros
                assert bool((bits[:, V:] == 0).all())
                assert bool((bits[~dead_rows][:, :V] != 0).any()) if bool((~dead_rows).any()) else True
                # a cotangent vector with g = 1 and a scalar g with c: the same bits when the products are equal
                assert torch.equal(run_backward(K, x, E, bias, labels, c * gval, lse, 1.0, V, T), dl)
                assert torch.equal(run_backward(K, x, E, bias, labels, c / 2, lse, 2 * gval, V, T), dl)
                release()
    print("sequence loss V=%d Vp=%d Hd=%d: worst loss_seq error / bound %.3f, total error / bound %.3f, worst dz error %.2e of max-abs (bound 6e-3)"
          % (V, Vp, Hd, worst["seq"], worst["total"], worst["dz"]))


def test_sequence_loss_wrappers_and_limits(K):
    V, Vp, Hd, S, T = 500, 512, 128, 6, 4
    E, bias = operands(V, Vp, Hd)
    x, labels, c = sequence_case(S, T, V, Hd, "all_ignored")
    lse, loss_seq, total = run_forward(K, x, E, bias, labels, V, S, T, c)
    w_seq, w_total, w_lse = K.mlm_seq_fwd(x, E, bias, labels, V, T, c)
    assert torch.equal(w_seq, loss_seq) and torch.equal(w_total, total) and torch.equal(w_lse, lse)
    assert K.mlm_seq_fwd(x, E, bias, labels, V, T)[1] is None
    g = torch.tensor([0.75], device=dev)
    assert torch.equal(K.mlm_seq_bwd(x, E, bias, labels, c, w_lse, g, V, T), run_backward(K, x, E, bias, labels, c, lse, 0.75, V, T))
    # lse is x2_ce_combine's, bit for bit
    _, lse_rows = K.mlm_ce_rows(x, E, bias, labels, V)
    assert torch.equal(lse_rows, w_lse)
    with pytest.raises(Exception, match="x2_seq_loss_combine"):
        K.call("x2_seq_loss_combine", K.ptr(x), 8, K.ptr(x), K.ptr(labels), 1, 128, None, K.ptr(x), K.ptr(x), None)
    with pytest.raises(Exception, match="x2_mlm_seq_bwd"):
        K.call("x2_mlm_seq_bwd", K.ptr(x), K.ptr(E), K.ptr(bias), K.ptr(labels), K.ptr(c), K.ptr(lse), K.ptr(g), 5, S * T, Vp, V, Hd, Hd, Hd,
               K.ptr(x), Vp)
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------------------------------------------- the decoder's forward(labels=...)

def test_decoder_forward_with_labels_at_tiny(synthetic, tmp_path):
    mg = importlib.import_module("x2-vlm_amd.model_generation")
    tc = VQA_TRAIN_CASES["tiny"]
    model = mg.XVLMForVQA(vqa_train_config("tiny", str(tmp_path)))
    synthetic.synth_state_dict(model, tc["wseed"])
    dec = model.to(dev).eval().text_decoder
    b = {k: v.to(dev) for k, v in vqa_train_batch(synthetic, "tiny").items()}
    ids, atts = b["answer_ids"], b["answer_atts"]
    S, La = ids.shape
    Hd = dec.config.hidden_size
    enc = torch.randn(S, 8, Hd, generator=torch.Generator().manual_seed(5)).to(dev)
    labels = ids.masked_fill(ids == 0, -100)
    out = dec(ids, attention_mask=atts, encoder_hidden_states=enc, labels=labels, reduction="none")
    assert out.loss.shape == (S,) and out.loss.dtype == F32 and out.loss.requires_grad and out.total is None
    assert out.last_hidden_state.shape == (S, La, Hd)
    with torch.no_grad():
        h = dec(ids, attention_mask=atts, encoder_hidden_states=enc).last_hidden_state
        assert torch.equal(h, out.last_hidden_state)
        rows = h[:, :-1].reshape(S * (La - 1), Hd).contiguous()
        nxt = labels[:, 1:].reshape(-1).contiguous()
        loss_rows, _ = dec.head_loss_rows(K_cast(rows), nxt)
        loss_rows = loss_rows.view(S, La - 1)
        acc = torch.zeros(S, device=dev)
        for t in range(La - 1):                                                 # index order, fp32: the kernel's order
            acc = acc + loss_rows[:, t]
        assert torch.equal(out.loss.detach(), acc), float((out.loss.detach() - acc).abs().max())
        mean = dec(ids, attention_mask=atts, encoder_hidden_states=enc, labels=labels).loss
        count = int((nxt >= 0).sum())
        want = float(loss_rows.double().sum()) / count
        assert mean.dim() == 0 and abs(float(mean) - want) <= 1e-6 * want
    # differentiable for an arbitrary cotangent: the weighted form's gradient when the cotangent is the weights
    w = torch.tensor([0.5, 1.0, 0.25, 0.0, 1.0, 0.75], device=dev)
    params = [p for p in dec.parameters()]
    out.loss.backward(w)
    first = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    out2 = dec(ids, attention_mask=atts, encoder_hidden_states=enc, reduction="none", _next_labels=labels[:, 1:].contiguous(), _seq_weights=w)
    assert torch.equal(out2.loss, out.loss.detach()) and not out2.loss.requires_grad and out2.total.requires_grad
    total = float(out2.total.detach())
    assert abs(total - float((w.double() * out.loss.detach().double()).sum())) <= 1e-6 * total
    out2.total.backward()
    for p, g0 in zip(params, first):                                           # the embedding scatter adds in no fixed order: not bit for bit
        assert float((p.grad - g0).abs().max()) <= 1e-5 * float(g0.abs().max()) + 1e-12
    print("decoder forward(labels) tiny: per-answer losses %s, mean %.6f" % ([round(float(v), 4) for v in out.loss.detach()], float(mean)))


def K_cast(rows):
    return importlib.import_module("x2-vlm_amd.kernels").cast_bf16(rows)
