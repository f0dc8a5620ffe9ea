"""Parity cases of the wide-label classification fine-tunes (XVLMForClassification, XVLMForVQAClassification), shared by make_golden_cls.py
(reference run, build container only) and the tests.  Geometry and batch from cases.CASES (cases.make_batch: the case's own batch size and seed);
weights, targets, k, weights and the KL teacher are regenerated from the seeds, so fixtures hold outputs only.

With synthetic weights the logits have a standard deviation of about 0.12 and the gap between a row's best and second-best logit is often below
0.01, less than the bf16 path's error: an argmax comparison would then test rounding noise.  The generator therefore asserts top2_margin >= MARGIN
for every row and the weight seeds are chosen so that this holds (for the two single-tower cases: the first seed >= 171 that does, pinned here);
a logits error below MARGIN / 2 cannot flip an argmax."""
from cases import CASES, make_batch, model_config

MARGIN = 0.02
CLS_CASES = {
    # VQA v2 over the closed answer set: k-expanded weighted cross-entropy (one row without answers, one ignored target, one duplicate), KL
    "tiny_vqacls": dict(model="vqa", case="tiny", labels=3129, wseed=179, k=[2, 0, 3, 1], ignore=1, duplicate=(4, 2)),
    # the task's real token geometry (384 px, N = 577, width 1024: the head is 1024 -> 2048 -> 3129)
    "large_shallow_vqacls": dict(model="vqa", case="large_shallow", labels=3129, wseed=174, k=[1, 2]),
    # VQA_msrvtt.py's 1500-way classifier on image batches, one ignored target
    "tiny_cls": dict(model="cls", case="tiny", labels=1500, wseed=179, ignore=2),
    # ... and on 5-D frame batches (frame position embedding, frame mean)
    "tiny_video_cls": dict(model="cls", case="tiny_video", labels=1500, wseed=179),
    # image=None: the CLS row of the 12-layer text pass
    "tiny_text_cls": dict(model="cls", case="tiny", labels=1500, wseed=172, branch="text"),
    # text_ids=None with task_name == 'imagenet': the vision CLS row, feature_dim = vision_width (768 -> 1536 -> 1000)
    "tiny_image_cls": dict(model="cls", case="tiny", labels=1000, wseed=171, branch="image", task_name="imagenet"),
}
TSEED = 181        # targets, weights and the teacher


def cls_config(name, workdir):
    cc = CLS_CASES[name]
    cfg = dict(model_config(cc["case"], workdir), num_labels=cc["labels"])
    if "task_name" in cc:
        cfg["task_name"] = cc["task_name"]
    return cfg


def cls_batch(synthetic, name, bseed=None, ragged=None):
    """The case's batch (CPU tensors): image, text_ids, text_atts (None where the branch takes none), targets int64 [T]; for the VQA model also
    k (list), weights fp32 [T] drawn from {0.1 .. 1.0} and answer_pred fp32 [B, C], the teacher logits of the KL mode."""
    import numpy as np
    import torch
    cc = CLS_CASES[name]
    c = dict(CASES[cc["case"]])
    if bseed is not None:
        c["bseed"] = bseed
    if ragged is not None:
        c["ragged"] = ragged
    b = make_batch(synthetic, c)
    B, C = c["batch"], cc["labels"]
    r = np.random.default_rng([TSEED, c["bseed"], C])
    out = dict(image=b["image"], text_ids=b["text_ids"], text_atts=b["text_atts"])
    if cc.get("branch") == "text":
        out["image"] = None
    if cc.get("branch") == "image":
        out["text_ids"] = out["text_atts"] = None
    T = sum(cc["k"]) if cc["model"] == "vqa" else B
    targets = r.integers(0, C, size=T)
    if "duplicate" in cc:
        targets[cc["duplicate"][0]] = targets[cc["duplicate"][1]]
    if "ignore" in cc:
        targets[cc["ignore"]] = -100
    out["targets"] = torch.from_numpy(targets.astype(np.int64))
    if cc["model"] == "vqa":
        assert len(cc["k"]) == B
        out["k"] = list(cc["k"])
        out["weights"] = torch.from_numpy((r.integers(1, 11, size=T) / 10.0).astype(np.float32))
        out["answer_pred"] = torch.from_numpy((2.0 * r.standard_normal((B, C))).astype(np.float32))
    return out


def top2_margin(logits):
    """min over rows of (best - second best) in float64"""
    import numpy as np
    l = np.sort(np.asarray(logits, dtype=np.float64), axis=1)
    return float((l[:, -1] - l[:, -2]).min())
