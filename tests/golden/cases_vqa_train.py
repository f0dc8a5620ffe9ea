"""VQA training-step parity cases, shared by make_golden_vqa_train.py (reference run, build container only) and the tests.  Geometry and model
configuration are cases_vqa's (cases.CASES underneath); weights and batches are regenerated from the seeds (x2-vlm_amd/synthetic.py), so the
fixtures hold outputs only."""
from cases import CASES
from cases_vqa import vqa_config

VQA_TRAIN_CASES = {
    # 2 + 2 layer text encoder, 2 decoder layers, V = 512: every op of the step in seconds on CPU
    "tiny": dict(case="tiny", batch=3, seq_len=8, k=[3, 1, 2], answer_len=5, num_dec_layers=2, wseed=51, bseed=152),
    # BERT-base widths (12 heads, d_h 64), V = 30522, 1 decoder layer
    "base_shallow": dict(case="base_shallow", batch=2, seq_len=30, k=[2, 3], answer_len=8, num_dec_layers=1, wseed=53, bseed=154),
}
WORD = "text_decoder.bert.embeddings.word_embeddings.weight"       # the tied parameter: lookup and LM head both contribute to its gradient
N_SAMPLE = 64


def vqa_train_config(name, workdir):
    cfg = vqa_config(name, workdir)
    assert cfg["num_dec_layers"] == VQA_TRAIN_CASES[name]["num_dec_layers"]
    return cfg


def vqa_train_batch(synthetic, name, k=None, bseed=None):
    tc = VQA_TRAIN_CASES[name]
    c = CASES[tc["case"]]
    return synthetic.synth_vqa_train_batch(tc["bseed"] if bseed is None else bseed, tc["batch"], tc["seq_len"], c["image_res"], c["vocab"],
                                           tc["k"] if k is None else k, tc["answer_len"])


def word_sample_index(answer_ids, hidden):
    """The fixed N_SAMPLE flat indices into the gradient of WORD [V, hidden]: the rows of the tokens that occur in the answers (sorted, the
    padding id 0 left out), walked round-robin, columns spread evenly over the hidden size.  -> list of ints."""
    tokens = sorted(set(int(t) for t in answer_ids.reshape(-1).tolist()) - {0})
    return [tokens[i % len(tokens)] * hidden + (i * (hidden - 1)) // (N_SAMPLE - 1) for i in range(N_SAMPLE)]
