"""Image-text retrieval on the MI355X stages.

  XVLMForRetrieval      models/model_retrieval.py:6-28   fine-tuning forward: (loss_itc, loss_itm) with `idx` soft labels; capturable
  rerank_scores         Retrieval.py:113-160             ITM re-ranking of the top-k ITC candidates, both directions
  retrieval_evaluation  Retrieval.py:71-168              features of all texts and images, then rerank_scores: the two device score matrices
  retrieval_eval        Retrieval.py:171-215 (itm_eval)  the nine recall figures from the device matrices: two launch pairs, one read-back

The reference re-ranks one query at a time: a fusion pass over k_test rows, the query's image tokens repeated k_test
times (i2t) or gathered per candidate (t2i).  Here `queries_per_pass` queries share one launch sequence and the image
K/V projections are computed once per DISTINCT image of the pass (kv_idx), never per pair: for i2t that is k_test x
fewer cross-attention K/V GEMM rows, the dominant cost of a fusion layer at L = 30 text tokens vs 197 image tokens.
"""
import torch
import torch.distributed as dist

from . import ops
from .xvlm import XVLMBase


class XVLMForRetrieval(XVLMBase):
    def __init__(self, config):
        super().__init__(config, load_vision_params=False, load_text_params=False, use_contrastive_loss=True,
                         use_matching_loss=True, use_mlm_loss=False, use_bbox_loss=False)
        self.num_attention_heads = self.text_encoder.config.num_attention_heads
        self.init_params = []

    def forward(self, image, text_ids, text_atts, idx=None):
        """image [B, 3, H, W], or [B, F, 3, H, W] for video retrieval (frames folded into the batch, get_vision_embeds)."""
        for t in (image, text_ids, text_atts) + (() if idx is None else (idx,)):
            ops.require_hip(t, "XVLMForRetrieval.forward")
        image_embeds, image_atts = self.get_vision_embeds(image)
        text_embeds = self.get_text_embeds(text_ids, text_atts)
        with torch.no_grad():
            self.temp.clamp_(0.001, 0.5)
        image_feat, text_feat = self.get_features(image_embeds, text_embeds)
        loss_itc = self.get_contrastive_loss(image_feat, text_feat, idx=idx)
        loss_itm = self.get_matching_loss(image_embeds, image_atts, image_feat, text_embeds, text_atts, text_feat, idx=idx)
        return loss_itc, loss_itm


def _shard(n, rank, world_size):
    step = n // world_size + 1                      # Retrieval.py:118-120
    start = rank * step
    return start, min(n, start + step)


@torch.no_grad()
def rerank_scores(model, image_feats, image_embeds, text_feats, text_atts, text_embeds, k_test, rank=0, world_size=1,
                  queries_per_pass=16, reduce=True):
    """Retrieval.py:113-160.  image_feats [Ni,T,D] / text_feats [Nt,L,Hd]: encoder outputs (the reference's naming);
    image_embeds [Ni,E] / text_embeds [Nt,E]: normalised ITC features.  Returns (score_i2t [Ni,Nt], score_t2i [Nt,Ni]),
    -100 outside each query's top-k; rows of other ranks are filled by the all-reduce when a process group exists."""
    was_training = model.training
    model.eval()
    dev = image_feats.device
    Ni, Nt = image_feats.shape[0], text_feats.shape[0]
    image_atts = torch.ones(image_feats.shape[:2], dtype=torch.long, device=dev)
    sims = ops.linear(image_embeds.float(), text_embeds.float())              # image_embeds @ text_embeds.t()
    score_i2t = torch.full((Ni, Nt), -100.0, device=dev)
    score_t2i = torch.full((Nt, Ni), -100.0, device=dev)

    def itm(images, atts, texts, tatts, t_idx, kv):
        cls = model._fusion_cls(images, atts, texts, tatts, t_idx.to(torch.int32), kv.to(torch.int32))
        return ops.mlp_head(model.itm_head, cls)[:, 1]

    start, end = _shard(Ni, rank, world_size)
    for q0 in range(start, end, queries_per_pass):
        q1 = min(end, q0 + queries_per_pass)
        topk = sims[q0:q1].topk(k=k_test, dim=1).indices                      # [nq, k] text ids
        nq = q1 - q0
        kv = torch.arange(nq, device=dev).repeat_interleave(k_test)           # pair -> image of the pass
        uniq, inv = torch.unique(topk.reshape(-1), return_inverse=True)       # pair -> text of the pass
        score = itm(image_feats[q0:q1], image_atts[q0:q1], text_feats[uniq], text_atts[uniq], inv, kv)
        score_i2t[q0:q1].scatter_(1, topk, score.view(nq, k_test))
    sims_t = sims.t()
    start, end = _shard(Nt, rank, world_size)
    for q0 in range(start, end, queries_per_pass):
        q1 = min(end, q0 + queries_per_pass)
        topk = sims_t[q0:q1].topk(k=k_test, dim=1).indices                    # [nq, k] image ids
        nq = q1 - q0
        uniq, inv = torch.unique(topk.reshape(-1), return_inverse=True)       # distinct images of the pass: K/V once each
        t_idx = torch.arange(nq, device=dev).repeat_interleave(k_test)
        score = itm(image_feats[uniq], image_atts[uniq], text_feats[q0:q1], text_atts[q0:q1], t_idx, inv)
        score_t2i[q0:q1].scatter_(1, topk, score.view(nq, k_test))
    if reduce and world_size > 1 and dist.is_available() and dist.is_initialized():
        # every entry is written by exactly one rank; the others hold -100 there (Retrieval.py:154-157 sums them as is)
        dist.barrier()
        dist.all_reduce(score_i2t, op=dist.ReduceOp.SUM)
        dist.all_reduce(score_t2i, op=dist.ReduceOp.SUM)
    model.train(was_training)
    return score_i2t, score_t2i


@torch.no_grad()
def _evaluation_features(model, image_batches, text_ids, text_atts, text_bs):
    """Retrieval.py:81-115: (image_feats [Ni, T, D], image_embeds [Ni, E], text_feats [Nt, L, Hd], text_embeds [Nt, E]) in eval mode - the
    encoder outputs and the normalised ITC features of all captions (text_bs at a time) and of all images (batch by batch)."""
    ops.require_hip(text_ids, "retrieval_evaluation")
    ops.require_hip(text_atts, "retrieval_evaluation")
    was_training = model.training
    model.eval()
    text_feats, text_embeds = [], []
    for i in range(0, text_ids.shape[0], text_bs):
        f = model.get_text_embeds(text_ids[i:i + text_bs], text_atts[i:i + text_bs])
        text_feats.append(f)
        text_embeds.append(model.get_features(text_embeds=f))
    image_feats, image_embeds = [], []
    for image in image_batches:
        ops.require_hip(image, "retrieval_evaluation")
        f, _ = model.get_vision_embeds(image)
        image_feats.append(f)
        image_embeds.append(model.get_features(image_embeds=f))
    model.train(was_training)
    return torch.cat(image_feats, 0), torch.cat(image_embeds, 0), torch.cat(text_feats, 0), torch.cat(text_embeds, 0)


@torch.no_grad()
def retrieval_evaluation(model, image_batches, text_ids, text_atts, k_test, text_bs=256, rank=0, world_size=1):
    """Retrieval.py:71-168 without tokenizer and loader: text_ids / text_atts [Nt, L] are the tokenised captions (device tensors), encoded in
    chunks of text_bs; image_batches is an iterable of device image batches ([b, 3, H, W], or [b, F, 3, H, W] for video) in dataset order.
    Then rerank_scores as it is.  Returns the two DEVICE matrices (score_i2t [Ni, Nt], score_t2i [Nt, Ni]); retrieval_eval reads them there."""
    image_feats, image_embeds, text_feats, text_embeds = _evaluation_features(model, image_batches, text_ids, text_atts, text_bs)
    return rerank_scores(model, image_feats, image_embeds, text_feats, text_atts, text_embeds, k_test, rank=rank, world_size=world_size)


def ground_truth_csr(ground_truth, rows):
    """(offs int32 [rows + 1], ids int32 [T]) host tensors from the reference's annotation tables: a dict or list of lists (img2txt: query ->
    its captions, possibly none) or a list of single ids (txt2img).  Queries of a dict that are missing have no ground truth."""
    offs, ids = [0], []
    for r in range(rows):
        if isinstance(ground_truth, dict):
            g = ground_truth.get(r, ())
        else:
            g = ground_truth[r]
        g = list(g) if isinstance(g, (list, tuple)) else [g]
        ids.extend(int(j) for j in g)
        offs.append(len(ids))
    return torch.tensor(offs, dtype=torch.int32), torch.tensor(ids, dtype=torch.int32)


RECALL_KEYS = ("txt_r1", "txt_r5", "txt_r10", "txt_r_mean", "img_r1", "img_r5", "img_r10", "img_r_mean", "r_mean")


def retrieval_eval(score_i2t, score_t2i, txt2img, img2txt):
    """itm_eval (Retrieval.py:171-215) on the device matrices: the CSR of both directions is built once on the host, ops.retrieval_ranks runs once
    per direction (two launches each) and the eight counts come back in ONE read.  rank = the number of scores STRICTLY greater than the ground
    truth's (csrc/retrieval.hip's tie rule: the reference's rank whenever the ground truth's score is not tied; R@1 / R@5 / R@10 equal for
    k_test >= 10).  Returns the reference's nine keys with its arithmetic (100.0 * count / len)."""
    ops.require_hip(score_i2t, "retrieval_eval")
    ops.require_hip(score_t2i, "retrieval_eval")
    dev = score_i2t.device
    counts = torch.zeros(2, 4, dtype=torch.int64, device=dev)
    for d, (scores, gt) in enumerate(((score_i2t, img2txt), (score_t2i, txt2img))):
        offs, ids = ground_truth_csr(gt, scores.shape[0])
        ops.retrieval_ranks(scores, offs.to(dev), ids.to(dev), counts[d])
    (t1, t5, t10, nt), (i1, i5, i10, ni) = counts.cpu().tolist()
    tr1, tr5, tr10 = 100.0 * t1 / nt, 100.0 * t5 / nt, 100.0 * t10 / nt
    ir1, ir5, ir10 = 100.0 * i1 / ni, 100.0 * i5 / ni, 100.0 * i10 / ni
    tr_mean, ir_mean = (tr1 + tr5 + tr10) / 3, (ir1 + ir5 + ir10) / 3
    return dict(zip(RECALL_KEYS, (tr1, tr5, tr10, tr_mean, ir1, ir5, ir10, ir_mean, (tr_mean + ir_mean) / 2)))
