"""Visual-grounding parity cases, shared by make_golden_grounding.py (reference run, build container only) and the tests.
Geometry from cases.CASES; weights, batches, target boxes and the evaluation set are regenerated from the seeds, so fixtures hold outputs
only.  tseed (the target boxes' seed) is chosen by make_golden_grounding.py --search so that, in every row of a non-degenerate case, every
quantity that passes through max / min / abs / clamp in the box tail is at least MARGIN from its kink; the generator asserts it."""
import numpy as np

from cases import CASES, model_config

GROUNDING_CASES = {
    "tiny": dict(case="tiny", wseed=111, tseed=8),
    # the task's real token geometry: 384 px, N = 577, width 1024
    "large_shallow": dict(case="large_shallow", wseed=113, tseed=1),
    # one target box of negative width: the reference's early-out zeroes every row's GIoU term
    "tiny_degenerate": dict(case="tiny", wseed=111, tseed=8, degenerate=True),
}
MARGIN = 2e-2                    # four times the project's coordinate bound of 5e-3 (tests/test_model_gpu.py POINTWISE["bbox_coord"])
EVAL_SEED, EVAL_N = 7, 96
SPLITS = ("val", "testA", "testB")


def grounding_config(name, workdir):
    return model_config(GROUNDING_CASES[name]["case"], workdir)


def target_boxes(tseed, batch):
    """Seeded target boxes [batch, 4] fp32, normalised cxcywh, inside the image."""
    r = np.random.default_rng([int(tseed), 0x67726E64])
    wh = r.uniform(0.15, 0.6, size=(batch, 2))
    c = r.uniform(0.0, 1.0, size=(batch, 2)) * (1.0 - wh) + wh / 2
    return np.concatenate([c, wh], axis=1).astype(np.float32)


def grounding_batch(synthetic, name, tseed=None):
    """The case's `bseed` image / text batch with its seeded target boxes (CPU tensors)."""
    import torch
    gc = GROUNDING_CASES[name]
    c = CASES[gc["case"]]
    b = synthetic.synth_batch(c["bseed"], c["batch"], c["seq_len"], c["image_res"], c["vocab"], c["max_masks"], ragged=c["ragged"])
    t = target_boxes(gc["tseed"] if tseed is None else tseed, c["batch"])
    if gc.get("degenerate"):
        t[1, 2] = -0.25
    return dict(image=b["image"], text_ids=b["text_ids"], text_atts=b["text_atts"], target_bbox=torch.from_numpy(t))


def xyxy(b):
    b = np.asarray(b, dtype=np.float64)
    return np.stack([b[:, 0] - 0.5 * b[:, 2], b[:, 1] - 0.5 * b[:, 3], b[:, 0] + 0.5 * b[:, 2], b[:, 1] + 0.5 * b[:, 3]], axis=1)


def kink_margin(coord, target):
    """The least distance (float64) of any quantity of the box tail from the kink of the max / min / abs / clamp it passes through, over all
    rows: the four coord - target components (abs), the four pairs of compared edges (max and min compare the same pairs), the two overlap
    extents and the two enclosing extents (clamp at 0)."""
    coord, target = np.asarray(coord, dtype=np.float64), np.asarray(target, dtype=np.float64)
    a, b = xyxy(coord), xyxy(target)
    overlap = np.minimum(a[:, 2:], b[:, 2:]) - np.maximum(a[:, :2], b[:, :2])
    hull = np.maximum(a[:, 2:], b[:, 2:]) - np.minimum(a[:, :2], b[:, :2])
    return float(min(np.abs(coord - target).min(), np.abs(a - b).min(), np.abs(overlap).min(), np.abs(hull).min()))


def pretrain_state(synthetic, names_shapes, seed=161):
    """The seeded synthetic pre-training checkpoint of the mapping test: one tensor per floating-point (name, shape)."""
    return {n: synthetic.synth_tensor(n, s, seed) for n, s in names_shapes}


def eval_set(seed=EVAL_SEED, n=EVAL_N):
    """A seeded evaluation set: pred fp32 [n, 4] normalised cxcywh, ref_box fp32 [n, 4] pixel xywh (two decimals, as COCO annotations),
    size fp32 [n, 2] (width, height), split labels.  Most predictions are the reference box moved and scaled by up to a third of its size (IoU
    spread on both sides of 0.5), every eighth is drawn independently (mostly low or zero overlap)."""
    r = np.random.default_rng([int(seed), 0x6576616C])
    size = np.stack([r.integers(320, 641, size=n), r.integers(240, 641, size=n)], axis=1).astype(np.float64)
    wh = r.uniform(0.15, 0.6, size=(n, 2)) * size
    xy = r.uniform(0.0, 1.0, size=(n, 2)) * (size - wh)
    ref = np.round(np.concatenate([xy, wh], axis=1), 2)
    pwh = ref[:, 2:] * r.uniform(0.67, 1.5, size=(n, 2))
    pc = ref[:, :2] + ref[:, 2:] / 2 + ref[:, 2:] * r.uniform(-0.33, 0.33, size=(n, 2))
    far = np.arange(n) % 8 == 7
    pwh[far] = (r.uniform(0.15, 0.6, size=(n, 2)) * size)[far]
    pc[far] = (r.uniform(0.2, 0.8, size=(n, 2)) * size)[far]
    pred = np.concatenate([pc / size, pwh / size], axis=1)
    split = [SPLITS[i] for i in r.integers(0, 3, size=n)]
    return pred.astype(np.float32), ref.astype(np.float32), size.astype(np.float32), split


def iou_float64(pred, ref_box, size):
    """grounding_eval_bbox's per-sample arithmetic and computeIoU (dataset/utils.py:363-453) restated in float64 on the given (fp32) inputs."""
    p, rb, s = (np.asarray(t, dtype=np.float64) for t in (pred, ref_box, size))
    pw, ph = p[:, 2] * s[:, 0], p[:, 3] * s[:, 1]
    px, py = p[:, 0] * s[:, 0] - pw / 2, p[:, 1] * s[:, 1] - ph / 2
    x1, y1 = np.maximum(rb[:, 0], px), np.maximum(rb[:, 1], py)
    x2, y2 = np.minimum(rb[:, 0] + rb[:, 2] - 1, px + pw - 1), np.minimum(rb[:, 1] + rb[:, 3] - 1, py + ph - 1)
    inter = np.where((x1 < x2) & (y1 < y2), (x2 - x1 + 1) * (y2 - y1 + 1), 0.0)
    return inter / (rb[:, 2] * rb[:, 3] + pw * ph - inter)
