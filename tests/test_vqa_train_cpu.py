"""CPU checks of the VQA training step (XVLMForVQA.forward(train=True), BertLMHeadModel.forward(labels=...)): what is refused and under which
words - host tensors ("training step" / "labels": the path is HIP only), label smoothing in the decoder loss, a host k that does not fit the
batch - all before anything is launched; synth_vqa_train_batch is deterministic and well formed; both goldens satisfy the reference's formula
loss == sum(weights * answer_loss) / B in float64 to 1e-6 and name exactly this repo's parameters; the library exports the three new entry
points under ABI 14 and refuses their limits without a launch."""
import ctypes
import importlib
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cases import CASES
from cases_vqa_train import N_SAMPLE, VQA_TRAIN_CASES, WORD, vqa_train_batch, vqa_train_config, word_sample_index

GOLD_DIR = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def mg():
    return importlib.import_module("x2-vlm_amd.model_generation")


def gold(name):
    return np.load("%s/%s_vqa_train.npz" % (GOLD_DIR, name))


def spaces(b):
    return (SimpleNamespace(input_ids=b["question_ids"], attention_mask=b["question_atts"]),
            SimpleNamespace(input_ids=b["answer_ids"], attention_mask=b["answer_atts"]))


def test_host_tensors_are_refused_as_the_training_step(mg, synthetic, tmp_path):
    model = mg.XVLMForVQA(vqa_train_config("tiny", str(tmp_path)))
    b = vqa_train_batch(synthetic, "tiny")
    q, a = spaces(b)
    with pytest.raises(NotImplementedError, match="training step.*HIP path"):
        model(b["image"], q, a, k=b["k"].tolist(), weights=b["weights"], train=True)
    with pytest.raises(NotImplementedError, match="labels.*HIP path"):
        model.text_decoder(b["answer_ids"], labels=b["answer_ids"])
    with pytest.raises(NotImplementedError, match="labels.*HIP path"):
        model.text_decoder(b["answer_ids"], labels=b["answer_ids"], reduction="none")
    with pytest.raises(NotImplementedError, match="return_logits"):
        model.text_decoder(b["answer_ids"], return_logits=True)


class _OnDevice(torch.Tensor):
    """A host tensor that reports is_cuda: the argument checks behind require_hip run on this machine and must raise before any launch (a
    launch on host memory would not raise NotImplementedError)."""

    @staticmethod
    def wrap(t):
        return t.as_subclass(_OnDevice)

    @property
    def is_cuda(self):
        return True


def test_argument_shapes_are_refused_before_any_launch(mg, synthetic, tmp_path, monkeypatch):
    model = mg.XVLMForVQA(vqa_train_config("tiny", str(tmp_path)))
    K = importlib.import_module("x2-vlm_amd.kernels")
    monkeypatch.setattr(K, "call", lambda *a, **kw: pytest.fail("a kernel was launched before the arguments were checked"))
    b = vqa_train_batch(synthetic, "tiny")
    q, a = spaces(b)
    image = _OnDevice.wrap(b["image"])
    S = b["answer_ids"].shape[0]
    for k in ([3, 1, 1], [3, 1, 2, 1], [3, 3], [4, 0, 2], [6, 1, -1]):                          # sum != S, len != B, an entry < 1
        with pytest.raises(NotImplementedError, match="training step"):
            model(image, q, a, k=k, weights=b["weights"], train=True)
    with pytest.raises(NotImplementedError, match="training step"):
        model(image, q, a, k=torch.tensor([3, 1, 1]), weights=b["weights"], train=True)       # a host tensor is checked like a list
    with pytest.raises(NotImplementedError, match="training step"):
        model(image, q, a, k=[3, 1, 2], weights=torch.ones(S - 1), train=True)
    with pytest.raises(NotImplementedError, match="training step"):
        model(image, q, a, k=[1], weights=torch.ones(1), train=True)                             # the call the ranking tests pin
    long_a = SimpleNamespace(input_ids=torch.ones(S, 129, dtype=torch.int64), attention_mask=torch.ones(S, 129, dtype=torch.int64))
    one_a = SimpleNamespace(input_ids=torch.ones(S, 1, dtype=torch.int64), attention_mask=torch.ones(S, 1, dtype=torch.int64))
    for bad in (long_a, one_a, None):
        with pytest.raises(NotImplementedError, match="training step"):
            model(image, q, bad, k=[3, 1, 2], weights=b["weights"], train=True)


def test_label_smoothing_in_the_decoder_loss_is_refused(tmp_path, synthetic, mg, monkeypatch):
    xbert = importlib.import_module("x2-vlm_amd.xbert")
    K = importlib.import_module("x2-vlm_amd.kernels")
    monkeypatch.setattr(K, "call", lambda *a, **kw: pytest.fail("a kernel was launched"))
    cfg = mg.XVLMForVQA(vqa_train_config("tiny", str(tmp_path))).text_decoder.config
    dec = xbert.BertLMHeadModel(cfg, label_smoothing=0.1)
    ids = _OnDevice.wrap(vqa_train_batch(synthetic, "tiny")["answer_ids"])
    with pytest.raises(NotImplementedError, match="label_smoothing"):
        dec(ids, labels=ids, reduction="none")
    with pytest.raises(NotImplementedError, match="label_smoothing"):
        dec(ids, labels=ids)


def test_synth_vqa_train_batch_is_deterministic_and_well_formed(synthetic):
    for name, tc in VQA_TRAIN_CASES.items():
        a, b = vqa_train_batch(synthetic, name), vqa_train_batch(synthetic, name)
        assert all(torch.equal(a[k], b[k]) for k in a)
        c = CASES[tc["case"]]
        ids, atts, S, La = a["answer_ids"], a["answer_atts"], sum(tc["k"]), tc["answer_len"]
        assert ids.shape == (S, La) and atts.shape == (S, La) and a["weights"].shape == (S,) and a["weights"].dtype == torch.float32
        assert a["k"].tolist() == tc["k"] and a["question_ids"].shape == (tc["batch"], tc["seq_len"]) and a["image"].shape[0] == tc["batch"]
        cls_id, sep_id = (101, 102) if c["vocab"] > 2000 else (1, 2)
        lens = atts.sum(1)
        assert bool((ids[:, 0] == cls_id).all()) and bool((ids.gather(1, (lens - 1).view(-1, 1)) == sep_id).all())
        assert bool(((ids == 0) == (atts == 0)).all())                                 # [SEP] is followed by 0s only, and no 0 comes earlier
        assert bool((atts[:, :-1] >= atts[:, 1:]).all())
        assert int(lens.min()) >= 3 and int(lens.max()) == La and len(set(lens.tolist())) > 1
        off = 0
        for n in tc["k"]:                                                              # no two rows of one question are equal
            assert len(set(map(tuple, ids[off:off + n].tolist()))) == n
            off += n
        allowed = set(np.array([0.3, 0.6, 0.9, 1.0], dtype=np.float32).tolist())
        assert set(a["weights"].tolist()) <= allowed and len(set(a["weights"].tolist())) > 1
        assert (a["question_atts"] == 0).any()
    other = vqa_train_batch(synthetic, "tiny", bseed=VQA_TRAIN_CASES["tiny"]["bseed"] + 1)
    assert not torch.equal(other["answer_ids"], vqa_train_batch(synthetic, "tiny")["answer_ids"])
    regrouped = vqa_train_batch(synthetic, "tiny", k=[2, 2, 2])
    assert regrouped["k"].tolist() == [2, 2, 2] and regrouped["answer_ids"].shape == (6, 5)
    for bad in ([3, 1], [3, 0, 3]):
        with pytest.raises(ValueError):
            vqa_train_batch(synthetic, "tiny", k=bad)


@pytest.mark.parametrize("name", list(VQA_TRAIN_CASES))
def test_golden_satisfies_the_reference_formula_and_names_this_models_parameters(mg, synthetic, name, tmp_path):
    g = gold(name)
    tc = VQA_TRAIN_CASES[name]
    b = vqa_train_batch(synthetic, name)
    assert g["k"].tolist() == tc["k"] and np.array_equal(g["weights"], b["weights"].numpy())
    S = sum(tc["k"])
    assert g["answer_loss"].shape == (S,) and g["word_sample"].shape == (N_SAMPLE,)
    want = float((g["weights"].astype(np.float64) * g["answer_loss"].astype(np.float64)).sum() / tc["batch"])
    assert abs(float(g["loss"]) - want) <= 1e-6 * abs(want)
    model = mg.XVLMForVQA(vqa_train_config(name, str(tmp_path)))
    mine = sorted(n for n, _ in model.named_parameters())
    assert mine == sorted(k[len("gradnorm/"):] for k in g.files if k.startswith("gradnorm/"))
    norms = np.array([float(g["gradnorm/" + n]) for n in mine])
    assert abs(float(np.sqrt((norms ** 2).sum())) - float(g["total_grad_norm"])) <= 1e-9 * float(g["total_grad_norm"])
    assert bool((norms > 0).all())
    # only the key biases' gradients are rounding noise (softmax is invariant to a shift of every score of a row)
    noise = [n for n, v in zip(mine, norms) if v < 1e-6 * float(g["total_grad_norm"])]
    assert noise and all(n.endswith("key.bias") for n in noise)
    # the sample sits in rows of tokens the answers use, where lookup and tied head both contribute
    hidden = dict(model.named_parameters())[WORD].shape[1]
    idx = word_sample_index(b["answer_ids"], hidden)
    used = set(b["answer_ids"].reshape(-1).tolist()) - {0}
    assert len(idx) == N_SAMPLE and len(set(idx)) == N_SAMPLE and all(i // hidden in used for i in idx)
    assert idx == word_sample_index(b["answer_ids"], hidden) and bool(np.abs(g["word_sample"]).max() > 0)


def test_library_exports_the_training_entry_points():
    lib = importlib.import_module("x2-vlm_amd._lib")
    K = importlib.import_module("x2-vlm_amd.kernels")
    h = lib.lib()
    for name in ("x2_vqa_train_rows", "x2_seq_loss_combine", "x2_mlm_seq_bwd"):
        assert name in lib.EXPORTS and hasattr(h, name) and getattr(h, name).argtypes is not None
    assert h.x2_abi_version() == 14
    for fn in ("vqa_train_rows", "mlm_seq_fwd", "mlm_seq_bwd"):
        assert callable(getattr(K, fn))
    one = ctypes.c_void_p(16)                 # any non-null address: the checks below return before anything is dereferenced
    assert h.x2_vqa_train_rows(one, one, one, one, 2, 6, 129, 0, one, one, one, 192, one, None) == -1 and b"La=129" in h.x2_last_error()
    assert h.x2_vqa_train_rows(one, one, one, one, 2, 6, 1, 0, one, one, one, 64, one, None) == -1
    assert h.x2_vqa_train_rows(one, one, one, one, 2, 6, 5, 0, one, one, one, 5, one, None) == -1 and b"mask2d_ld" in h.x2_last_error()
    assert h.x2_vqa_train_rows(one, one, one, one, 0, 6, 5, 0, one, one, one, 64, one, None) == -1
    assert h.x2_vqa_train_rows(one, one, one, None, 2, 6, 5, 0, one, one, one, 64, one, None) == -1
    assert h.x2_seq_loss_combine(one, 8, one, one, 4, 128, None, one, one, None, None) == -1 and b"x2_seq_loss_combine" in h.x2_last_error()
    assert h.x2_seq_loss_combine(one, 8, one, one, 4, 0, None, one, one, None, None) == -1
    assert h.x2_seq_loss_combine(one, 8, one, one, 4, 4, one, one, one, None, None) == -1 and b"come together" in h.x2_last_error()
    assert h.x2_mlm_seq_bwd(one, one, None, one, one, one, one, 4, 10, 512, 512, 128, 128, 128, one, 512, None) == -1       # R % T != 0
    assert b"x2_mlm_seq_bwd" in h.x2_last_error()
    assert h.x2_mlm_seq_bwd(one, one, None, one, one, one, one, 4, 8, 512, 512, 128, 128, 128, one, 504, None) == -1        # ldd < Vp
    assert h.x2_mlm_seq_bwd(one, one, None, one, one, one, one, 4, 8, 500, 500, 128, 128, 128, one, 512, None) == -1        # Vp not padded to 64
