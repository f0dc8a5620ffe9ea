"""Differentiable functional ops on the HIP kernels for the small heads and glue of the step
(projection + F.normalize, build_mlp heads, cross-entropies, row gathers, region pooling)."""
import torch

from . import kernels as K
from .engine import (BANK, CrossEntropyFn, GatherRowsFn, GeluF32Fn, L2NormFn, LayerNormF32Fn, LinearBf16Fn, LinearF32Fn)


def linear(x, w, b=None):
    return LinearF32Fn.apply(x, w, b)


def layer_norm(x, w, b, eps):
    return LayerNormF32Fn.apply(x, w, b, eps)


def gelu(x):
    return GeluF32Fn.apply(x)


def normalize(x):
    return L2NormFn.apply(x)


def cross_entropy(logits, labels):
    return CrossEntropyFn.apply(logits, labels)


def gather_rows(src, idx):
    return GatherRowsFn.apply(src, idx.to(torch.int32))


_HOST_PATH = "%s runs on the HIP path; a host (CPU) path is a possible follow-up and is not implemented"


def require_hip(t, who):
    """the entry points without a host path: anything but a HIP tensor is refused under the caller's name"""
    if not isinstance(t, torch.Tensor) or not t.is_cuda: raise NotImplementedError(_HOST_PATH % who)


def mlp_head(seq, x):
    """nn.Sequential(Linear, LayerNorm(1e-5), GELU, Linear) of xvlm.py:163-169 on fp32 rows."""
    w0 = seq[0].weight
    if w0.shape[1] % 64 == 0 and w0.shape[0] % 8 == 0 and x.numel() % 4 == 0:
        h = LinearBf16Fn.apply(x, w0, seq[0].bias)          # 768 -> 1536: MFMA GEMM
    else:
        h = linear(x, w0, seq[0].bias)
    h = gelu(layer_norm(h, seq[1].weight, seq[1].bias, seq[1].eps))
    return linear(h, seq[3].weight, seq[3].bias)


def head_first_linear(seq, x):
    """seq[0] of a build_mlp head, for the heads whose tail is cls_tail / cls_wide.  The condition is mlp_head's, word for word, and the two
    copies must change together; folding mlp_head onto this function is pending (it is on the pretraining step's path)."""
    w0 = seq[0].weight
    if w0.shape[1] % 64 == 0 and w0.shape[0] % 8 == 0 and x.numel() % 4 == 0:
        return LinearBf16Fn.apply(x, w0, seq[0].bias)
    return linear(x, w0, seq[0].bias)


class _MaskedMeanToken0(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w):
        out = x.contiguous().clone()
        w = w.contiguous()
        K.pool_tokens(out, w)
        ctx.save_for_backward(w)
        return out

    @staticmethod
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        g = dy.contiguous().clone()
        K.pool_tokens(g, w, bwd=True)
        return g, None


def masked_mean_token0(x, w):
    """token 0 <- sum_p w[b,p] x[b,1+p] / sum_p w[b,p]   (region pooling, beit2.py:430-436)."""
    return _MaskedMeanToken0.apply(x, w)


class _FrameMean(torch.autograd.Function):
    """(B*F, T, D) + pos (1,F,1,D) -> mean over frames (B, T, D).  xvlm.py:627-645; x2_frame_mean forward / backward kernels
    (HBM-bound row work)."""

    @staticmethod
    def forward(ctx, x, pos, frames):
        BF, T, D = x.shape
        ctx.frames, ctx.pos_shape = frames, pos.shape
        if not x.is_cuda:                                        # host use (unit tests of the wrapper logic): plain tensor maths
            return (x.view(BF // frames, frames, T, D).sum(1) + pos.view(1, frames, 1, D).sum(1)) / frames
        return K.frame_mean(x.contiguous(), pos.detach().reshape(frames, D).contiguous(), frames)

    @staticmethod
    def backward(ctx, dy):
        f = ctx.frames
        B, T, D = dy.shape
        if not dy.is_cuda:
            g = (dy / f).unsqueeze(1).expand(B, f, T, D).reshape(B * f, T, D)
            return g, (dy.sum((0, 1)) / f).view(1, 1, 1, D).expand(1, f, 1, D).clone(), None
        dx, dpos = K.frame_mean_bwd(dy.contiguous(), f)
        return dx, dpos.view(ctx.pos_shape), None


def frame_mean(x, pos, frames):
    return _FrameMean.apply(x, pos, frames)


class _BboxLoss(torch.autograd.Function):
    """sigmoid + L1 + GIoU of matched pairs (xvlm.py:923, 927-957) as kernels.bbox_loss_fwd / _bwd: two launches for the whole box tail.
    Nothing is read back: the degenerate flag and the box count stay in `stat` on the device, so the function can be captured."""

    @staticmethod
    def forward(ctx, logits, target, keep):
        coord, stat = K.bbox_loss_fwd(logits.contiguous(), target, keep)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(coord, target, keep, stat)
        return coord, stat[0], stat[1]

    @staticmethod
    def backward(ctx, g_coord, g_bbox, g_giou):
        coord, target, keep, stat = ctx.saved_tensors
        if g_coord is None and g_bbox is None and g_giou is None:
            return None, None, None
        scalar = lambda g: None if g is None else g.to(torch.float32).reshape(1).contiguous()
        return K.bbox_loss_bwd(coord, target, keep, stat, scalar(g_bbox), scalar(g_giou),
                               None if g_coord is None else g_coord.to(torch.float32).contiguous()), None, None


def bbox_loss(logits, target, is_image=None):
    """(output_coord, loss_bbox, loss_giou) of XVLMBase.get_bbox_loss applied to bbox_head's logits [B, 4]: output_coord = sigmoid(logits),
    the L1 and GIoU means over the rows with is_image == 0 (all rows when None).  Differentiable in logits, through all three outputs."""
    target = target.detach().to(torch.float32).contiguous()
    keep = None if is_image is None else (1 - is_image).detach().to(torch.float32).contiguous()
    return _BboxLoss.apply(logits, target, keep)


def _head_rows(h):
    """h as the row kernels read it: unit column stride, a row stride that is a multiple of 4, a 16-byte aligned base"""
    return h.contiguous() if h.stride(-1) != 1 or h.stride(0) % 4 or h.data_ptr() % 16 else h


def _head_cotangents(g_loss, g_logits):
    """(g_loss as a device scalar fp32 [1], g_logits as contiguous fp32), None staying None"""
    return (None if g_loss is None else g_loss.to(torch.float32).reshape(1).contiguous(),
            None if g_logits is None else g_logits.to(torch.float32).contiguous())


class _ClsTail(torch.autograd.Function):
    """LayerNorm -> GELU -> Linear(H -> C) [-> F.cross_entropy(ignore_index=-100)] behind a head's first Linear as kernels.cls_tail_fwd /
    _bwd: at most two launches each way.  Only h, the logits and the per-row {mean, rstd} are kept for the backward; n_valid stays in `stat` on
    the device and nothing is read back, so the function can be captured."""

    @staticmethod
    def forward(ctx, h, gamma, beta, w, bias, eps, labels):
        h = _head_rows(h)
        logits, rowstat, _, stat = K.cls_tail_fwd(h, gamma.detach().contiguous(), beta.detach().contiguous(), w.detach().contiguous(),
                                                  bias.detach().contiguous(), eps, labels)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, gamma, beta, w, rowstat, logits, labels, stat)
        return logits, (stat[0] if labels is not None else None)

    @staticmethod
    def backward(ctx, g_logits, g_loss):
        h, gamma, beta, w, rowstat, logits, labels, stat = ctx.saved_tensors
        if g_logits is None and g_loss is None:
            return (None,) * 7
        g_loss, g_logits = _head_cotangents(g_loss, g_logits)
        dh, dgamma, dbeta, dw, dbias = K.cls_tail_bwd(h, gamma.detach().contiguous(), beta.detach().contiguous(), w.detach().contiguous(), rowstat,
                                                      logits, labels, stat, g_loss, g_logits)
        return dh, dgamma, dbeta, dw, dbias, None, None


def cls_tail(seq, h, targets=None):
    """(logits [R, C], loss | None) of a build_mlp head's tail seq[1] (LayerNorm), seq[2] (GELU), seq[3] (Linear) on the rows h = seq[0](x), the
    loss being F.cross_entropy(logits, targets, ignore_index=-100) when targets are given.  Differentiable through both outputs."""
    require_hip(h, "ops.cls_tail")
    labels = None if targets is None else targets.detach().to(torch.int64).contiguous()
    return _ClsTail.apply(h, seq[1].weight, seq[1].bias, seq[3].weight, seq[3].bias, seq[1].eps, labels)


class _ClsWide(torch.autograd.Function):
    """LayerNorm -> GELU -> Linear(H -> C) with C in the hundreds or thousands, and one of three losses on its logits: none, the cross-entropy with
    several weighted targets per row (entries offs[r] .. offs[r+1]-1 of targets / weights), or the KL divergence to a dense teacher.  The logits
    are the MFMA GEMM of the bf16 activation (kernels.lngelu_fwd) with the zero-padded bf16 weight (BANK.vocab, Cp = C rounded up to 64: the pad
    columns hold 0 and no kernel reads them); the losses, their bf16 dlogits and LayerNorm -> GELU's backward are csrc/classify_wide.hip, the input
    and weight gradients the GEMMs the MLM decoder uses.  Kept for the backward: h, act, {mean, rstd}, the padded logits and the per-row
    statistics; the denominator stays in `stat` on the device and nothing is read back, so the function can be captured."""

    @staticmethod
    def forward(ctx, h, gamma, beta, w, bias, eps, offs, targets, weights, teacher, denom_mode):
        h = _head_rows(h)
        R, C = h.shape[0], w.shape[0]
        act, rowstat = K.lngelu_fwd(h, gamma.detach().contiguous(), beta.detach().contiguous(), eps)
        Wp, _ = BANK.vocab(w)
        Cp = Wp.shape[0]
        bias_p = BANK.vector(bias, Cp - C) if Cp > C else bias.detach()
        logits = K.gemm_nt(act, Wp, bias=bias_p, out_dtype=torch.float32)
        lse = lse_t = stat = None
        if teacher is not None:
            ctx.mode = 2
            lse, lse_t, _, stat = K.kl_ce_fwd(logits, teacher, C)
        elif targets is not None:
            ctx.mode = 1
            lse, _, stat = K.soft_ce_fwd(logits, C, offs, targets, weights, denom_mode)
        else:
            ctx.mode = 0
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(h, gamma, beta, w, act, rowstat, logits, offs, targets, weights, teacher, lse, lse_t, stat)
        return logits[:, :C], (stat[0] if stat is not None else None)

    @staticmethod
    def backward(ctx, g_logits, g_loss):
        h, gamma, beta, w, act, rowstat, logits, offs, targets, weights, teacher, lse, lse_t, stat = ctx.saved_tensors
        if g_logits is None and g_loss is None:
            return (None,) * 11
        BANK.note_backward()
        R, H = h.shape
        C = w.shape[0]
        g_loss, g_logits = _head_cotangents(g_loss, g_logits)
        _, WpT = BANK.vocab(w)
        Cp = WpT.shape[1]
        if ctx.mode == 2:
            dl = K.kl_ce_bwd(R, C, logits=logits, teacher=teacher, lse=lse, lse_t=lse_t, g_loss=g_loss, g_logits=g_logits, Cp=Cp)
        elif ctx.mode == 1:
            dl = K.soft_ce_bwd(R, C, logits=logits, offs=offs, targets=targets, weights=weights, lse=lse, stat=stat, g_loss=g_loss,
                               g_logits=g_logits, Cp=Cp)
        else:
            dl = K.soft_ce_bwd(R, C, g_logits=g_logits, Cp=Cp)
        dact = K.gemm_nt(dl, WpT, out_dtype=torch.float32)
        dw = torch.empty_like(w)
        K.gemm_tn_grouped([(dl, act, dw, Cp, H)])
        dbias_p = torch.zeros(Cp, device=h.device, dtype=torch.float32)
        K.colsum_bf16(dl, dbias_p)
        dh, dgamma, dbeta = K.lngelu_bwd(dact, h, gamma.detach().contiguous(), beta.detach().contiguous(), rowstat)
        return dh, dgamma, dbeta, dw, dbias_p[:C], None, None, None, None, None, None


def cls_wide(seq, h, *, targets=None, offs=None, weights=None, teacher=None, denom_mode=0):
    """(logits [R, C], loss | None) of a build_mlp head's tail seq[1] (LayerNorm), seq[2] (GELU), seq[3] (Linear, any number of labels) on the rows
    h = seq[0](x).  The loss, by what is given:
      teacher fp32 [R, C]         KLDivLoss('none')(log_softmax(logits), softmax(teacher)).sum() / R
      targets int64 [T] with offs int32 [R + 1] (row r owns entries offs[r] .. offs[r+1]-1) and weights fp32 [T] or None (= 1):
                                  sum_r sum_j w_j * CE(logits[r], t_j) / denom; an entry outside [0, C) (the -100 of ignore_index) is skipped;
                                  denom_mode 0: denom = R, 1: the number of non-skipped entries (none at all gives NaN, as F.cross_entropy does)
      neither                     None
    Differentiable through both outputs; nothing is read back.  The caller guarantees 0 <= offs[r] <= offs[r+1] <= T."""
    require_hip(h, "ops.cls_wide")
    H = seq[1].weight.numel()
    if H % 64:
        raise ValueError("ops.cls_wide: the hidden width H=%d of the head must be a multiple of 64 (the contraction of the logits GEMM)" % H)
    R = h.shape[0]
    if teacher is not None:
        teacher = teacher.detach().to(torch.float32)
        if teacher.dim() != 2 or teacher.shape != (R, seq[3].weight.shape[0]):
            raise ValueError("ops.cls_wide: teacher must be [R, C] = [%d, %d]" % (R, seq[3].weight.shape[0]))
        if teacher.stride(1) != 1:
            teacher = teacher.contiguous()
        targets = offs = weights = None
    elif targets is not None:
        targets = targets.detach().to(torch.int64).contiguous().view(-1)
        if offs is None:
            raise ValueError("ops.cls_wide: targets need offs (int32 [R + 1])")
        offs = offs.detach().to(torch.int32).contiguous()
        weights = None if weights is None else weights.detach().to(torch.float32).contiguous().view(-1)
        if offs.shape != (R + 1,) or (weights is not None and weights.shape != targets.shape):
            raise ValueError("ops.cls_wide: offs must be [R + 1] and weights as long as targets")
    return _ClsWide.apply(h, seq[1].weight, seq[1].bias, seq[3].weight, seq[3].bias, seq[1].eps, offs, targets, weights, teacher, denom_mode)


class _ItcSoft(torch.autograd.Function):
    """The soft-label contrastive loss (xvlm.py:805-826) as kernels.itc_soft_fwd / _bwd: two launches forward, one backward.  Kept for the
    backward: the logits, the ids and the per-row / per-column {lse, cnt}.  Nothing is read back, so the function can be captured."""

    @staticmethod
    def forward(ctx, logits, idx):
        out, rowstat, colstat, _ = K.itc_soft_fwd(logits, idx)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(logits, idx, rowstat, colstat)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        logits, idx, rowstat, colstat = ctx.saved_tensors
        if g is None:
            return None, None
        return K.itc_soft_bwd(logits, idx, rowstat, colstat, g.to(torch.float32).reshape(1).contiguous()), None


def itc_soft(logits, idx_all):
    """(mean_i CE(logits[i], lab[i]) + mean_j CE(logits[:, j], lab[j])) / 2 with lab = pos / pos.sum(1), pos = (idx_all == idx_all^T): the `idx`
    branch of XVLMBase.get_contrastive_loss on fp32 logits [N, N] (similarities / temp, 2 <= N <= 1024) and the gathered ids [N].
    Differentiable in logits; nothing is read back."""
    require_hip(logits, "ops.itc_soft")
    require_hip(idx_all, "ops.itc_soft")
    if logits.dim() != 2 or logits.shape[0] != logits.shape[1] or idx_all.numel() != logits.shape[0]:
        raise ValueError("ops.itc_soft: logits must be [N, N] and idx_all hold N ids (got %s and %d)" % (tuple(logits.shape), idx_all.numel()))
    logits = logits.to(torch.float32)
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    return _ItcSoft.apply(logits, idx_all.detach().to(torch.int64).reshape(-1).contiguous())


def retrieval_ranks(scores, gt_offs, gt_ids, counts):
    """ranks int32 [R] of fp32 device scores [R, N] under the CSR ground truths (gt_offs int32 [R + 1], gt_ids int32), counts int64 [4] +=
    {#ranks < 1, #ranks < 5, #ranks < 10, R}: kernels.retrieval_ranks (rank = the number of STRICTLY greater scores; INT_MAX without a ground
    truth).  No read-back."""
    require_hip(scores, "ops.retrieval_ranks")
    scores = scores.detach().to(torch.float32)
    if scores.stride(1) != 1:
        scores = scores.contiguous()
    return K.retrieval_ranks(scores, gt_offs, gt_ids, counts)
