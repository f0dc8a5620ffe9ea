"""Captioning inference: the reference's beam search (models/model_generation.py:139-397, from unilm s2s-ft) on the HIP path.

The reference keeps every layer's input states of the prefix and re-projects their K/V each step over image tokens repeated per beam.
Here a step feeds [chosen token, [MASK]] (the first step: prompt + [MASK]) through the text stack with
  * a per-row, per-layer K/V cache indexed by ABSOLUTE position (kernels.attn_decode: the [MASK] of step t writes slot next_pos, the token
    chosen at t has that same position and overwrites it at t + 1 - the reference's dropping of the [MASK] state, without a copy),
  * the cross-attention K/V of the image tokens projected once per image per layer and shared by the beams through kv_idx,
  * the MLM head on the [MASK] rows only (the text encoder's head_logits, xbert.LMHeadRows), scored by kernels.logprob_topk (log-softmax,
    n-gram and EOS penalties, top-K: one launch, no host round trip), and the caches reordered by the back pointers in one launch for
    all layers (kernels.beam_gather, ping-pong buffers).
The beam bookkeeping (merge_beams) is torch on the device, without a host sync inside the loop; one transfer after it feeds backtrace().
merge_beams and backtrace are pure functions usable on CPU tensors / lists; log_scores_reference and banned_tokens restate the scoring rule
on the host for the tests."""
import math

import torch

from . import kernels as K
from .engine import BANK, BertLayersFn
from .xbert import _key_mask

BF16, F32 = torch.bfloat16, torch.float32
MAX_NEW = 16          # x2_attn_decode: tokens per step (prompt + [MASK] at the first step)
MAX_LEN = 128         # x2_attn_decode: cache positions


# ----------------------------------------------------------------------------- pure host / torch pieces

def banned_tokens(seq, n):
    """Tokens that would complete a repeated n-gram of `seq` (list of ids): seq[i + n - 1] for every i with seq[i .. i+n-2] equal to the last
    n - 1 ids; none when len(seq) < n (get_dup_ngram_candidates with an empty forbid_ignore_set).  Sorted, without duplicates."""
    if n < 1 or len(seq) < n:
        return []
    tail = list(seq[len(seq) - (n - 1):]) if n > 1 else []
    return sorted({seq[i + n - 1] for i in range(len(seq) - (n - 1)) if list(seq[i:i + n - 1]) == tail})


def log_scores_reference(logits, seqs=None, ngram=0, eos_id=0, forbid_eos=False):
    """float64 restatement of kernels.logprob_topk's scores: log_softmax of logits [S, V], -10000 ADDED once per banned token of the row's ids
    so far (seqs: list of S id lists), column eos_id SET to -10000 when forbid_eos."""
    out = torch.log_softmax(logits.double(), -1).clone()
    if seqs is not None and ngram:
        for r, seq in enumerate(seqs):
            for tok in banned_tokens(list(seq), ngram):
                if 0 <= tok < out.shape[1]:
                    out[r, tok] += -10000.0
    if forbid_eos:
        out[:, eos_id] = -10000.0
    return out


def merge_beams(kk_scores, kk_ids, last_scores, last_eos, K_):
    """One step's selection from the per-row candidates.  kk_scores / kk_ids [S, K]: each row's K best log-scores and their ids.  First step
    (last_scores None, S = B): they are the beams.  Later (S = B * K): kk_scores += last_eos * -10000 + last_scores per parent beam, the K
    best of each image's K * K candidates (ties: lowest candidate index).  -> (k_scores [B, K], k_ids [B, K], back_ptrs [B, K] int64,
    merged [B, K * K] or None)."""
    if last_scores is None:
        B = kk_scores.shape[0]
        return kk_scores, kk_ids.long(), torch.zeros(B, K_, dtype=torch.long, device=kk_scores.device), None
    B = last_scores.shape[0]
    merged = (kk_scores + (last_eos.reshape(B * K_, 1) * -10000.0 + last_scores.reshape(B * K_, 1))).reshape(B, K_ * K_)
    order = torch.sort(merged, dim=1, descending=True, stable=True).indices[:, :K_]
    k_scores = torch.gather(merged, 1, order)
    back = torch.div(order, K_, rounding_mode="floor")
    k_ids = torch.gather(kk_ids.long().reshape(B, K_ * K_), 1, order)
    return k_scores, k_ids, back, merged


def _forced_scores(merged_or_scores, kk_ids, k_ids, back, K_):
    """Scores of a given (teacher-forced) selection: each forced id is looked up among its parent's K candidates; NaN where bf16 noise pushed
    it out of them.  Test seam only: a forced run makes no choice of its own, and its total scores (and with them the returned ids) carry
    no meaning wherever a NaN entered."""
    B = k_ids.shape[0]
    cand = kk_ids.long().reshape(B, -1, K_)
    if cand.shape[1] == 1:                                                # first step: one row per image
        back = torch.zeros_like(back)
    hit = torch.gather(cand, 1, back.unsqueeze(-1).expand(B, K_, K_)) == k_ids.unsqueeze(-1)
    found = torch.gather(merged_or_scores.reshape(B, -1), 1, back * K_ + hit.to(torch.int64).argmax(-1))
    return torch.where(hit.any(-1), found, torch.full_like(found, float("nan")))


def backtrace(total_scores, step_ids, back_ptrs, eos_id, length_penalty=0, output_length=None):
    """Captions from the recorded search, on the host: arrays [T, B, K] (anything numpy.asarray takes) of total scores, chosen ids and back
    pointers.  Per image the search ends at the first step whose beams are all EOS (else at the last step).  Candidates are the EOS
    entries up to that step and every entry of that step; with length_penalty > 0 a candidate of step t is scored total / ((6 + t) / 6) **
    length_penalty.  The best candidate wins, the earliest (step, beam) among equals, and its ids are read back through the pointers.
    -> id lists, zero-padded to output_length when given ([0] for an image without a finite candidate)."""
    import numpy as np
    score = np.asarray(total_scores, dtype=np.float64)
    token = np.asarray(step_ids, dtype=np.int64)
    parent = np.asarray(back_ptrs, dtype=np.int64)
    T, B, Kb = token.shape
    ended = token == eos_id
    done = ended.all(axis=2)                                              # [T, B]
    stop = np.where(done.any(axis=0), done.argmax(axis=0), T - 1)         # [B] the step that closes each image's search
    step = np.arange(T).reshape(T, 1, 1)
    if length_penalty > 0:
        score = score / np.power((6.0 + step) / 6.0, length_penalty)
    eligible = (step <= stop.reshape(1, B, 1)) & (ended | (step == stop.reshape(1, B, 1)))
    ranked = np.where(eligible, score, -np.inf).transpose(1, 0, 2).reshape(B, T * Kb)    # row-major (step, beam): argmax keeps the earliest
    captions = []
    for b in range(B):
        best = int(ranked[b].argmax())
        if not ranked[b, best] > -np.inf:
            path = [0]
        else:
            t, k = divmod(best, Kb)
            path = [0] * (t + 1)
            while True:
                path[t] = int(token[t, b, k])
                if t == 0:
                    break
                k = int(parent[t, b, k])
                t -= 1
        captions.append(path + [0] * max(0, (output_length or 0) - len(path)))
    return captions


def check_lengths(prompt_len, output_length, max_position_embeddings):
    """Refusals shared by generate / beam_search; -> number of decode steps (output_length - prompt_len)."""
    if output_length > max_position_embeddings:
        raise ValueError("generate: length %d exceeds max_position_embeddings %d" % (output_length, max_position_embeddings))
    if output_length > MAX_LEN:
        raise ValueError("generate: length %d exceeds the K/V cache's Lmax %d" % (output_length, MAX_LEN))
    if not 1 <= prompt_len < MAX_NEW:
        raise ValueError("generate: a prompt of %d tokens (with [CLS]) does not fit the first step's %d (prompt + [MASK])" % (prompt_len, MAX_NEW))
    if output_length <= prompt_len:
        raise ValueError("generate: length %d leaves no step after the %d prompt tokens" % (output_length, prompt_len))
    return output_length - prompt_len


def generation_lengths(bsz, prompt_len, max_length, max_position_embeddings):
    """generate()'s sizes, as the reference has them (model_generation.py:116-119): length = input_ids.size(0) + max_length, the BATCH size
    plus max_length.  -> (length, steps = length - prompt_len = bsz + max_length - prompt_len); raises what check_lengths refuses."""
    length = bsz + max_length
    return length, check_lengths(prompt_len, length, max_position_embeddings)


# ----------------------------------------------------------------------------- the decode step on the device

class _TextStack:
    """The text encoder's layers for decode steps: weights through the engine's WeightBank, the image tokens' cross-attention K/V projected
    once, two K/V cache buffers [layers, S, Lmax, 2 * Hd]."""

    def __init__(self, model, image_embeds, S, K_, Lmax):
        te = model.text_encoder
        self.te, self.cfg = te, te.config
        cfg = self.cfg
        self.H, self.Hd, self.eps = cfg.num_attention_heads, cfg.hidden_size, cfg.layer_norm_eps
        assert self.Hd == 64 * self.H, "hidden size %d / %d heads: the attention kernels are built for head dim 64" % (self.Hd, self.H)
        self.scale = 1.0 / math.sqrt(self.Hd // self.H)
        self.NL, self.fusion_at = cfg.num_hidden_layers, cfg.fusion_layer
        self.p = dict(te.bert.encoder.named_parameters())
        self.S, self.K, self.Lmax = S, K_, Lmax
        dev = image_embeds.device
        self.dev = dev
        BertLayersFn.prepare_weights(self.p, 0, self.NL, self.fusion_at, True)
        Bi, T, Dv = image_embeds.shape
        self.Bi, self.T = Bi, T
        encb = K.cast_bf16(image_embeds.contiguous().view(Bi * T, Dv))
        self.kv = {}
        for i in range(self.fusion_at, self.NL):                         # once per image and layer: the beams share them through kv_idx
            c = "layer.%d.crossattention." % i
            wkv, _ = BANK.linear(self.p[c + "self.key.weight"], self.p[c + "self.value.weight"])
            self.kv[i] = K.gemm_nt(encb, wkv, bias=BANK.vector(self.p[c + "self.key.bias"], self.p[c + "self.value.bias"]))
        self.caches = [torch.empty(self.NL, S, Lmax, 2 * self.Hd, device=dev, dtype=BF16) for _ in range(2)]
        self.cur = 0
        # image masks are all ones (get_image_embeds): additive key masks of zeros, per row count
        self.enc_mask = {n: _key_mask(torch.ones(n, T, dtype=torch.long, device=dev), -1e9) for n in {Bi, S}}
        kv_idx = (torch.arange(S, device=dev, dtype=torch.int32) // K_).contiguous()
        off, order = K.kv_csr(kv_idx, Bi)
        self.share = dict(kv_idx=kv_idx, seq_off=off, seq_ids=order)
        self.mask_rows = {}

    def step(self, ids, pids, hist):
        """ids / pids int64 [R, n_new] (R = Bi at the first step, else S) at absolute positions hist .. hist + n_new - 1 -> fp32 logits
        [R, Vp] of each row's last token (the [MASK]).  Launches per layer: QKV GEMM, attn_decode, output GEMM, LayerNorm, in fusion layers
        query GEMM + attention + output GEMM + LayerNorm, two FFN GEMMs, LayerNorm."""
        te, p, Hd, H, eps, dev = self.te, self.p, self.Hd, self.H, self.eps, self.dev
        R, n_new = ids.shape
        M = R * n_new
        h = te.bert.embeddings(ids, pids).view(M, Hd)
        hb = K.cast_bf16(h)
        cache = self.caches[self.cur]
        for i in range(self.NL):
            b = "layer.%d." % i
            a = b + "attention."
            wqkv, _ = BANK.linear(p[a + "self.query.weight"], p[a + "self.key.weight"], p[a + "self.value.weight"])
            bqkv = BANK.vector(p[a + "self.query.bias"], p[a + "self.key.bias"], p[a + "self.value.bias"])
            qkv = K.gemm_nt(hb, wqkv, bias=bqkv)
            att = K.attn_decode(qkv, cache[i][:R], R, H, n_new, hist, self.scale)
            wo, _ = BANK.linear(p[a + "output.dense.weight"])
            s1 = K.gemm_nt(att, wo, bias=p[a + "output.dense.bias"], resid=h, out_dtype=F32)
            hb, h, _, _ = K.layernorm_fwd(s1, p[a + "output.LayerNorm.weight"], p[a + "output.LayerNorm.bias"], eps, want_f32=True)
            if i >= self.fusion_at:
                c = b + "crossattention."
                wq, _ = BANK.linear(p[c + "self.query.weight"])
                q2 = K.gemm_nt(hb, wq, bias=p[c + "self.query.bias"])
                att2 = torch.empty(M, Hd, device=dev, dtype=BF16)
                lse2 = torch.empty(R * H * n_new, device=dev, dtype=F32)
                share = self.share if R == self.S and R != self.Bi else {}
                K.attn_fwd(K.view3(q2, R, n_new), K.view3(self.kv[i], self.Bi, self.T, 0), K.view3(self.kv[i], self.Bi, self.T, Hd), R, self.Bi,
                           H, n_new, self.T, self.scale, K.view3(att2, R, n_new), lse2, mask=self.enc_mask[R], **share)
                wo2, _ = BANK.linear(p[c + "output.dense.weight"])
                s2 = K.gemm_nt(att2, wo2, bias=p[c + "output.dense.bias"], resid=h, out_dtype=F32)
                hb, h, _, _ = K.layernorm_fwd(s2, p[c + "output.LayerNorm.weight"], p[c + "output.LayerNorm.bias"], eps, want_f32=True)
            wi, _ = BANK.linear(p[b + "intermediate.dense.weight"])
            wout, _ = BANK.linear(p[b + "output.dense.weight"])
            pre = torch.empty(M, wi.shape[0], device=dev, dtype=BF16)
            act = K.gemm_nt(hb, wi, bias=p[b + "intermediate.dense.bias"], aux=pre, act=1)
            s3 = K.gemm_nt(act, wout, bias=p[b + "output.dense.bias"], resid=h, out_dtype=F32)
            hb, h, _, _ = K.layernorm_fwd(s3, p[b + "output.LayerNorm.weight"], p[b + "output.LayerNorm.bias"], eps, want_f32=True)
        rows = self.mask_rows.get((R, n_new))
        if rows is None:
            rows = self.mask_rows[(R, n_new)] = (torch.arange(R, device=dev, dtype=torch.int32) * n_new + (n_new - 1)).contiguous()
        _, rb = K.gather_rows(h, rows, Hd, want_f32=False, want_bf16=True)
        return te.head_logits(rb)

    def reorder(self, parent, hist):
        """caches[l][s][:hist] <- caches[l][parent[s]][:hist] into the other buffer, which becomes the current one."""
        K.beam_gather(self.caches[self.cur], self.caches[1 - self.cur], parent, hist)
        self.cur = 1 - self.cur


def _uncached_logits(model, image_embeds, ids, pids, kv_idx):
    """The same step through the existing full-sequence forward (every step recomputes the whole prefix with the tril [R, L, L] mask): the
    baseline of probes/bench_captioning_generate.py and the tests' check of the cache."""
    te = model.text_encoder
    R, L = ids.shape
    atts = torch.tril(torch.ones(L, L, dtype=torch.long, device=ids.device)).expand(R, L, L)
    enc_atts = torch.ones(R, image_embeds.shape[1], dtype=torch.long, device=ids.device)
    h = te.bert(ids, attention_mask=atts, position_ids=pids, encoder_hidden_states=image_embeds, encoder_attention_mask=enc_atts,
                kv_idx=kv_idx).last_hidden_state
    return te.head_logits(K.cast_bf16(h[:, -1, :].contiguous()))


@torch.no_grad()
def beam_search(model, image, input_ids, token_type_ids, position_ids, attention_mask, num_beams=3, min_length=5, length_penalty=0,
                forbid_duplicate_ngrams=True, ngram_size=3, _forced=None, _return_traces=False, _use_cache=True):
    """See XVLMForMLMCaptioning.beam_search.  The model is already in eval mode."""
    eos_id, mask_id = model.generation_token_ids()
    cfg = model.text_encoder.config
    V = cfg.vocab_size
    dev = image.device
    B, P = input_ids.shape
    Lout = token_type_ids.shape[1]
    K_ = int(num_beams)
    if not 1 <= K_ <= 8:
        raise ValueError("beam_search: num_beams %d outside 1..8" % K_)
    steps = check_lengths(P, Lout, cfg.max_position_embeddings)
    if token_type_ids.shape[0] != B or position_ids.shape != (B, Lout) or attention_mask.shape != (B, Lout, Lout):
        raise ValueError("beam_search: token_type_ids / position_ids / attention_mask must be [B, length] / [B, length] / [B, length, length]")
    tril = torch.tril(torch.ones(Lout, Lout, dtype=attention_mask.dtype, device=dev))
    if not bool((attention_mask == tril).all()) or bool(token_type_ids.any()):
        raise NotImplementedError("beam_search: the K/V-cached decode step supports the tril attention mask and token type 0 of generate() only")
    S = B * K_
    Lmax = K.round_up(Lout, 8)
    image_embeds, _ = model.get_vision_embeds(image)
    stack = _TextStack(model, image_embeds, S, K_, Lmax) if _use_cache else None
    pos_b = position_ids.to(torch.int64)
    pos_s = pos_b.repeat_interleave(K_, 0)                                    # first_expand
    mask_col = torch.full((S, 1), mask_id, dtype=torch.int64, device=dev)
    prompt = input_ids.to(torch.int64)
    ngram = int(ngram_size) if forbid_duplicate_ngrams else 0
    seq = torch.zeros(S, K.round_up(steps, 4), dtype=torch.int32, device=dev)  # generated ids per beam
    base = (torch.arange(B, device=dev) * K_).unsqueeze(1)
    first_parent = (torch.arange(S, device=dev, dtype=torch.int32) // K_).contiguous()
    share_idx = first_parent if K_ > 1 else None
    last_scores = last_eos = None
    rec_scores, rec_ids, rec_ptrs, traces = [], [], [], []
    next_pos = P
    for t in range(steps):
        if t == 0:
            ids = torch.cat([prompt, mask_col[:B]], 1).contiguous()
            pids = pos_b[:, :P + 1].contiguous()
            hist = 0
        else:
            ids = torch.cat([k_ids.reshape(S, 1), mask_col], 1).contiguous()
            pids = pos_s[:, next_pos - 1:next_pos + 1].contiguous()
            hist = next_pos - 1
        if _use_cache:
            logits = stack.step(ids, pids, hist)
        elif t == 0:
            logits = _uncached_logits(model, image_embeds, ids, pids, None)
        else:
            full = torch.cat([prompt.repeat_interleave(K_, 0), seq[:, :t].long(), mask_col], 1).contiguous()
            logits = _uncached_logits(model, image_embeds, full, pos_s[:, :next_pos + 1].contiguous(), share_idx)
        forbid_eos = bool(min_length) and (next_pos - P + 1 <= min_length)
        want_logs = _return_traces and V <= 1024
        vals, cols, logs = K.logprob_topk(logits, V, K_, seq=seq if t else None, seq_len=t, ngram=ngram, eos_id=eos_id, forbid_eos=forbid_eos,
                                          want_logs=want_logs)
        k_scores, k_ids, back, merged = merge_beams(vals, cols, last_scores, last_eos, K_)
        if _forced is not None:
            k_ids = torch.as_tensor(_forced[0][t], dtype=torch.int64, device=dev).reshape(B, K_)
            back = torch.as_tensor(_forced[1][t], dtype=torch.int64, device=dev).reshape(B, K_)
            k_scores = _forced_scores(vals if merged is None else merged, cols, k_ids, back, K_)
        if _return_traces:
            traces.append(dict(vals=vals, ids=cols, logs=logs, logits=logits[:, :V]))
        rec_scores.append(k_scores)
        rec_ids.append(k_ids)
        rec_ptrs.append(back)
        last_scores, last_eos = k_scores, (k_ids == eos_id).to(k_scores.dtype)
        parent = first_parent if t == 0 else (base + back).reshape(S).to(torch.int32).contiguous()
        if t > 0:
            seq = seq.index_select(0, parent.long())
        seq[:, t] = k_ids.reshape(S).to(torch.int32)
        if _use_cache and t + 1 < steps:
            stack.reorder(parent, next_pos)                                   # positions 0 .. next_pos - 1: the [MASK]'s slot is not kept
        next_pos += 1
    packed = torch.stack([torch.stack(rec_scores).double(), torch.stack(rec_ids).double(), torch.stack(rec_ptrs).double()]).cpu()   # the one transfer
    total_scores, step_ids, back_ptrs = packed[0].float(), packed[1].long(), packed[2].long()
    pred = backtrace(total_scores.tolist(), step_ids.tolist(), back_ptrs.tolist(), eos_id, length_penalty, Lout)
    if _return_traces:
        return pred, dict(steps=traces, total_scores=total_scores, step_ids=step_ids, back_ptrs=back_ptrs)
    return pred
