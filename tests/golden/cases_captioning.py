"""Captioning fine-tune parity cases, shared by make_golden_captioning.py (reference run, build container only) and the tests.
Geometry from cases.CASES; weights and batches are regenerated from the seeds (x2-vlm_amd/synthetic.py), so fixtures hold outputs only."""
import os

from cases import CASES, model_config

CAP_CASES = {
    # every op of the path in seconds on CPU; full [B, n_mask, V] prediction scores kept
    "tiny": dict(case="tiny", batch=3, max_tokens=12, max_masks=4, wseed=41, bseed=5),
    # BERT-base widths (12 heads, d_h 64), V = 30522, the shipped text geometry: L = 40 + 18 = 58 in the FG-free form
    "base_shallow": dict(case="base_shallow", batch=2, max_tokens=40, max_masks=18, wseed=43, bseed=7),
}
LABEL_SMOOTHING = 0.1
SCORE_COLS = list(range(0, 30522, 97))                 # fixed column sample of the [B, n_mask, 30522] scores
GRAD_SAMPLE = {                                        # 64 evenly spaced gradient elements of these tensors
    "pos": "text_encoder.bert.embeddings.position_embeddings.weight",
    "word": "text_encoder.bert.embeddings.word_embeddings.weight",
    "q0": "text_encoder.bert.encoder.layer.0.attention.self.query.weight",
    "ckv": "text_encoder.bert.encoder.layer.2.crossattention.self.key.weight",
    "dec_bias": "text_encoder.cls.predictions.bias",
    "patch": "vision_encoder.patch_embed.proj.weight",
}


def caption_config(case, workdir):
    cfg = model_config(case, workdir)
    big = CASES[case]["vocab"] > 2000
    cfg.update(label_smoothing=LABEL_SMOOTHING, prompt="", cls_token_id=101 if big else 1)
    return cfg


def write_vocab(tdir, vocab):
    """vocab.txt of `vocab` entries whose [PAD] / [UNK] / [CLS] / [SEP] / [MASK] ids are those of synthetic.py's batches."""
    special = {0: "[PAD]", 100: "[UNK]", 101: "[CLS]", 102: "[SEP]", 103: "[MASK]"} if vocab > 2000 else \
        {0: "[PAD]", 1: "[CLS]", 2: "[SEP]", 3: "[MASK]", 4: "[UNK]"}
    with open(os.path.join(tdir, "vocab.txt"), "w") as f:
        for i in range(vocab):
            f.write(special.get(i, "w%d" % i) + "\n")
