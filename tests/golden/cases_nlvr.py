"""NLVR2 parity cases, shared by make_golden_nlvr.py (reference run, build container only) and the tests.  Geometry from cases.CASES; weights
and batches are regenerated from the seeds, so fixtures hold outputs only.  A case of B pairs draws ONE synthetic batch of 2B rows: its images
are image0 stacked over image1 (NLVR.py:44), its first B text rows are the statements; targets[i] = i % 2.  The generator asserts that the two
logits of every row are at least MARGIN apart, so a bf16 error in the logits of less than half of it cannot flip an argmax."""
from cases import CASES, model_config

NLVR_CASES = {
    "tiny": dict(case="tiny", wseed=171, pairs=4),
    # the task's real token geometry: 384 px, N = 577, width 1024
    "large_shallow": dict(case="large_shallow", wseed=171, pairs=2),
    # one ignored target: the mean runs over the other three rows
    "tiny_ignore": dict(case="tiny", wseed=171, pairs=4, ignore=1),
}
MARGIN = 0.15


def nlvr_config(name, workdir):
    return model_config(NLVR_CASES[name]["case"], workdir)


def nlvr_batch(synthetic, name, bseed=None, ragged=None):
    """The case's batch (CPU tensors): image [2B, 3, res, res], text_ids / text_atts [B, L], targets int64 [B]."""
    import torch
    nc = NLVR_CASES[name]
    c = CASES[nc["case"]]
    B = nc["pairs"]
    b = synthetic.synth_batch(c["bseed"] if bseed is None else bseed, 2 * B, c["seq_len"], c["image_res"], c["vocab"], c["max_masks"],
                              ragged=c["ragged"] if ragged is None else ragged)
    targets = torch.arange(B, dtype=torch.int64) % 2
    if "ignore" in nc:
        targets[nc["ignore"]] = -100
    return dict(image=b["image"], text_ids=b["text_ids"][:B].clone(), text_atts=b["text_atts"][:B].clone(), targets=targets)


def logit_margin(logits):
    """min over rows of |l0 - l1| in float64"""
    import numpy as np
    l = np.asarray(logits, dtype=np.float64)
    return float(np.abs(l[:, 0] - l[:, 1]).min())


def pretrain_state(synthetic, names_shapes, seed=173):
    """The seeded synthetic pre-training checkpoint of the mapping test: one tensor per floating-point (name, shape)."""
    return {n: synthetic.synth_tensor(n, s, seed) for n, s in names_shapes}
