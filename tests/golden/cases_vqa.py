"""VQA answer-ranking parity cases, shared by make_golden_vqa.py (reference run, build container only) and the tests.
Geometry from cases.CASES; weights and batches are regenerated from the seeds (x2-vlm_amd/synthetic.py), so fixtures hold outputs only.
aseed (the answer list's seed) is chosen by make_golden_vqa.py --search so that no first-stage cut splits a tie group, the cut margin
exceeds four times the first token's score bound and no two candidate rows are equal; the generator asserts all three."""
from cases import CASES, model_config

VQA_CASES = {
    # 2 + 2 layer text encoder, 2 decoder layers, V = 512: every op of the path in seconds on CPU
    "tiny": dict(case="tiny", batch=3, seq_len=8, n_answers=40, answer_len=5, k=8, num_dec_layers=2, wseed=51, bseed=52, aseed=363),
    # BERT-base widths (12 heads, d_h 64), V = 30522, 1 decoder layer
    "base_shallow": dict(case="base_shallow", batch=2, seq_len=30, n_answers=300, answer_len=8, k=32, num_dec_layers=1, wseed=53, bseed=54, aseed=2608402),
}
# load_pretrained key mapping: (text layers, fusion start, decoder layers) of the tiny geometry - the decoder as deep as the cross layers,
# and half as deep (4 cross layers)
MAP_FORMS = {"full": (4, 2, 2), "half": (6, 2, 2)}
PER_TOKEN = 2 * 1.5e-2          # x maxabs0: the log-score bound per scored token (tests/test_captioning_generate_gpu.py)


def vqa_config(name, workdir, text_layers=None, fusion_at=None, num_dec_layers=None):
    vc = VQA_CASES[name]
    cfg = model_config(vc["case"], workdir)
    if text_layers is not None:
        cfg.update(text_num_hidden_layers=text_layers, text_fusion_start_at=fusion_at)
    cfg.update(pad_token_id=0, num_dec_layers=vc["num_dec_layers"] if num_dec_layers is None else num_dec_layers)
    return cfg


def vqa_batch(synthetic, name, aseed=None):
    vc = VQA_CASES[name]
    c = CASES[vc["case"]]
    return synthetic.synth_vqa_batch(vc["bseed"], vc["batch"], vc["seq_len"], c["image_res"], c["vocab"], vc["n_answers"], vc["answer_len"],
                                     answer_seed=vc["aseed"] if aseed is None else aseed)


def pretrain_state(synthetic, names_shapes, seed=61):
    """The seeded synthetic pre-training checkpoint of the mapping test: one tensor per floating-point (name, shape)."""
    return {n: synthetic.synth_tensor(n, s, seed) for n, s in names_shapes}


def first_stage(logp_first, k):
    """The first stage's rule on the host: per row the k largest values, largest first, lowest candidate index first among equals.
    -> (values [B, k], ids [B, k]) as numpy arrays (float64 / int64)."""
    import numpy as np
    lp = np.asarray(logp_first, dtype=np.float64)
    order = np.stack([np.lexsort((np.arange(lp.shape[1]), -row))[:k] for row in lp])
    return np.take_along_axis(lp, order, 1), order


def second_stage(scores, ids):
    """The second stage's tail on the host (float64): softmax over a question's k scores, sorted by score, lowest slot first among
    equals -> (topk_probs [B, k], topk_ids [B, k])."""
    import numpy as np
    sc = np.asarray(scores, dtype=np.float64)
    order = np.stack([np.lexsort((np.arange(sc.shape[1]), -row)) for row in sc])
    e = np.exp(sc - sc.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)
    return np.take_along_axis(p, order, 1), np.take_along_axis(np.asarray(ids, dtype=np.int64), order, 1)
