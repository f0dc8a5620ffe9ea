"""Retrieval fine-tune parity cases, shared by make_golden_retrieval_step.py (reference run, build container only) and the tests.
Geometry from cases.CASES; weights, batches, `idx` and the injected negatives are regenerated from the seeds, so fixtures hold outputs only.
Every case carries its own batch size: the soft labels need groups of more than one row and a singleton, and every row needs a candidate with
another id to inject as its negative."""
import numpy as np

from cases import CASES, model_config

RETRIEVAL_CASES = {
    # two groups of two rows and one singleton
    "tiny": dict(case="tiny", batch=5, idx=[3, 5, 5, 9, 3], wseed=191, bseed=192),
    # the task's real token geometry: 384 px, N = 577, width 1024 (cases.CASES' own batch of 2 would leave a row without a negative)
    "large_shallow": dict(case="large_shallow", batch=3, idx=[7, 7, 2], wseed=193, bseed=194),
    # video retrieval: 5-D frame batches through the same class
    "tiny_video": dict(case="tiny_video", batch=3, idx=[1, 4, 1], wseed=195, bseed=196),
}

# the evaluation set of tests/golden/tiny_retrieval.npz (6 images, 10 captions, k_test = 4): its annotation tables, image 3 without a caption
EVAL_IMG2TXT = {0: [0, 1], 1: [2], 2: [3, 4, 5], 3: [], 4: [6, 7], 5: [8, 9]}
EVAL_TXT2IMG = [0, 0, 1, 2, 2, 2, 4, 4, 5, 5]


def retrieval_config(name, workdir):
    return model_config(RETRIEVAL_CASES[name]["case"], workdir)


def retrieval_negatives(idx, seed):
    """Injected hard negatives (image_neg_idx, text_neg_idx) as synthetic.synth_negatives gives them, but drawn among the rows with ANOTHER id:
    what get_hard_negatives(idx=...) can return."""
    r = np.random.default_rng([int(seed), 0x6E656773])
    idx = list(idx)
    out = []
    for _ in range(2):
        neg = []
        for b in range(len(idx)):
            cand = [j for j in range(len(idx)) if idx[j] != idx[b]]
            assert cand, "row %d has no candidate with another idx" % b
            neg.append(int(cand[int(r.integers(0, len(cand)))]))
        out.append(neg)
    return out[0], out[1]


def retrieval_batch(synthetic, name, bseed=None):
    """The case's batch (CPU tensors): image ([B, 3, H, W] or [B, F, 3, H, W]), text_ids, text_atts, idx int64 [B], negatives (two lists)."""
    import torch
    rc = RETRIEVAL_CASES[name]
    c = CASES[rc["case"]]
    seed = rc["bseed"] if bseed is None else bseed
    b = synthetic.synth_batch(seed, rc["batch"], c["seq_len"], c["image_res"], c["vocab"], c["max_masks"], ragged=c["ragged"], frames=c["frames"])
    return dict(image=b["image"], text_ids=b["text_ids"], text_atts=b["text_atts"], idx=torch.tensor(rc["idx"], dtype=torch.int64),
                negatives=retrieval_negatives(rc["idx"], seed))


def ranks_float64(scores, gt, N=None):
    """The declared rank rule restated on the host: per row the least, over its ground-truth columns inside [0, N), number of columns c < N whose
    score is STRICTLY greater; 2^31 - 1 for a row without one.  scores: [R, >= N]; gt: per row a list of column ids."""
    s = np.asarray(scores, dtype=np.float64)
    N = s.shape[1] if N is None else N
    out = np.full(s.shape[0], 2 ** 31 - 1, dtype=np.int64)
    for r in range(s.shape[0]):
        for j in gt[r]:
            if 0 <= j < N:
                out[r] = min(out[r], int((s[r, :N] > s[r, j]).sum()))
    return out


def recall_from_ranks(ranks_i2t, ranks_t2i):
    """itm_eval's nine figures (Retrieval.py:186-214) from the two rank vectors"""
    def three(ranks):
        return [100.0 * int((np.asarray(ranks) < k).sum()) / len(ranks) for k in (1, 5, 10)]
    tr, ir = three(ranks_i2t), three(ranks_t2i)
    tm, im = (tr[0] + tr[1] + tr[2]) / 3, (ir[0] + ir[1] + ir[2]) / 3
    return dict(txt_r1=tr[0], txt_r5=tr[1], txt_r10=tr[2], txt_r_mean=tm, img_r1=ir[0], img_r5=ir[1], img_r10=ir[2], img_r_mean=im,
                r_mean=(tm + im) / 2)
