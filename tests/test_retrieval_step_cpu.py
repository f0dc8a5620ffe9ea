"""CPU checks of the retrieval fine-tune step and evaluation (csrc/retrieval.hip, x2-vlm_amd/model_retrieval.py): the library exports the four
new entry points under ABI 14 with the header's signatures and refuses arguments outside the documented ranges without a launch; the cases of
cases_retrieval regenerate bit for bit and every row of every case has a negative with another id; the CSR of the ground truths is built from
the reference's ragged annotation tables (an image without captions included); host tensors are refused under the caller's name; the committed
fixtures hold the documented keys and nothing large."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest
import torch

from cases import CASES
from cases_retrieval import (EVAL_IMG2TXT, EVAL_TXT2IMG, RETRIEVAL_CASES, ranks_float64, recall_from_ranks, retrieval_batch,
                             retrieval_config, retrieval_negatives)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_DIR = os.path.join(ROOT, "tests", "golden")
NEW = {
    "x2_itc_soft_fwd": "const float* logits, int ld, const long* idx, int N, float* rowstat, float* colstat, float* loss_rows, float* out, void* stream",
    "x2_itc_soft_bwd": "const float* logits, int ld, const long* idx, int N, const float* rowstat, const float* colstat, const float* g, "
                       "float* dlogits, int ldd, void* stream",
    "x2_sample_negatives_checked": "const float* sim, int n, const long* group, const float* u, int* out, int* no_negative, void* stream",
    "x2_retrieval_ranks": "const float* scores, int ld, int R, int N, const int* gt_offs, const int* gt_ids, int* ranks, long* counts, void* stream",
}


@pytest.fixture(scope="module")
def mr():
    return importlib.import_module("x2-vlm_amd.model_retrieval")


def test_library_exports_the_retrieval_entry_points_with_the_header_signatures():
    lib = importlib.import_module("x2-vlm_amd._lib")
    K = importlib.import_module("x2-vlm_amd.kernels")
    ops = importlib.import_module("x2-vlm_amd.ops")
    h = lib.lib()
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "x2vlm_hip.h")).read(), flags=re.S))
    for name, args in NEW.items():
        assert "int %s(%s);" % (name, args) in header, name
        assert name in lib.EXPORTS and hasattr(h, name)
        want = [ctypes.c_void_p if "*" in a else ctypes.c_int for a in args.split(", ")]
        assert list(getattr(h, name).argtypes) == want and lib._SIGS[name] == want, name
    assert h.x2_abi_version() == 14
    for fn in ("itc_soft_fwd", "itc_soft_bwd", "sample_negatives_checked", "retrieval_ranks"):
        assert callable(getattr(K, fn))
    assert callable(ops.itc_soft) and callable(ops.retrieval_ranks)


def test_argument_checks_refuse_without_launching():
    """every check returns before anything is dereferenced or launched (no GPU here)"""
    h = importlib.import_module("x2-vlm_amd._lib").lib()
    one, byte = ctypes.c_void_p(16), ctypes.c_void_p(18)

    def refused(rc, name, word=None):
        msg = h.x2_last_error()
        assert rc == -1 and name in msg and (word is None or word in msg), (rc, msg)

    def fwd(N=8, ld=None, lg=one, idx=one, out=one):
        return h.x2_itc_soft_fwd(lg, N if ld is None else ld, idx, N, one, one, one, out, None)

    def bwd(N=8, ld=None, ldd=None, lg=one, g=one, dl=one):
        return h.x2_itc_soft_bwd(lg, N if ld is None else ld, one, N, one, one, g, dl, N if ldd is None else ldd, None)

    def smp(n=8, sim=one, flags=one):
        return h.x2_sample_negatives_checked(sim, n, None, one, one, flags, None)

    def rk(R=4, N=8, ld=None, sc=one, offs=one, counts=one, ranks=one):
        return h.x2_retrieval_ranks(sc, N if ld is None else ld, R, N, offs, one, ranks, counts, None)

    for N in (-1, 0, 1, 1025, 4096):
        refused(fwd(N=N), b"x2_itc_soft_fwd", b"N=")
        refused(bwd(N=N), b"x2_itc_soft_bwd", b"N=")
        refused(smp(n=N), b"x2_sample_negatives_checked", b"n=")
    refused(fwd(ld=7), b"x2_itc_soft_fwd", b"ld=")
    refused(bwd(ld=7), b"x2_itc_soft_bwd", b"ld=")
    refused(bwd(ldd=7), b"x2_itc_soft_bwd", b"ldd=")
    refused(fwd(lg=None), b"x2_itc_soft_fwd", b"null")
    refused(fwd(idx=None), b"x2_itc_soft_fwd", b"null")
    refused(fwd(out=None), b"x2_itc_soft_fwd", b"null")
    refused(bwd(g=None), b"x2_itc_soft_bwd", b"null")
    refused(bwd(dl=None), b"x2_itc_soft_bwd", b"null")
    refused(fwd(lg=byte), b"x2_itc_soft_fwd", b"aligned")
    refused(bwd(dl=byte), b"x2_itc_soft_bwd", b"aligned")
    refused(smp(sim=None), b"x2_sample_negatives_checked", b"null")
    refused(smp(flags=None), b"x2_sample_negatives_checked", b"null")
    for R in (0, -3):
        refused(rk(R=R), b"x2_retrieval_ranks", b"R=")
    for N in (0, -1, 65537):
        refused(rk(N=N), b"x2_retrieval_ranks", b"N=")
    refused(rk(ld=7), b"x2_retrieval_ranks", b"ld=")
    refused(rk(offs=None), b"x2_retrieval_ranks", b"null")
    refused(rk(counts=None), b"x2_retrieval_ranks", b"null")
    refused(rk(ranks=None), b"x2_retrieval_ranks", b"null")
    refused(rk(sc=byte), b"x2_retrieval_ranks", b"aligned")


def test_cases_regenerate_and_every_row_has_a_negative(synthetic, mr):
    """The cases themselves (a self-check of cases_retrieval), and their groups through the project's CSR builder: a row's positives, as a table
    row -> rows sharing its id, come back as the CSR whose every row holds the row itself."""
    assert sorted(RETRIEVAL_CASES) == ["large_shallow", "tiny", "tiny_video"]
    assert RETRIEVAL_CASES["tiny"]["idx"] == [3, 5, 5, 9, 3] and RETRIEVAL_CASES["large_shallow"]["idx"] == [7, 7, 2]
    assert RETRIEVAL_CASES["tiny_video"]["idx"] == [1, 4, 1]
    for name, rc in RETRIEVAL_CASES.items():
        c = CASES[rc["case"]]
        a, b = retrieval_batch(synthetic, name), retrieval_batch(synthetic, name)
        for k in ("image", "text_ids", "text_atts", "idx"):
            assert torch.equal(a[k], b[k]), (name, k)
        assert a["negatives"] == b["negatives"]
        B = rc["batch"]
        assert a["image"].shape[0] == B and a["image"].dim() == (5 if c["frames"] else 4) and a["idx"].tolist() == rc["idx"]
        if c["frames"]:
            assert a["image"].shape[1] == c["frames"]
        for neg in a["negatives"]:
            assert len(neg) == B
            for row, j in enumerate(neg):
                assert 0 <= j < B and rc["idx"][j] != rc["idx"][row], (name, row, j)
        groups = {r: [j for j in range(B) if rc["idx"][j] == rc["idx"][r]] for r in range(B)}
        offs, ids = mr.ground_truth_csr(groups, B)
        assert offs.tolist() == [0] + np.cumsum([len(groups[r]) for r in range(B)]).tolist() and ids.numel() == sum(len(v) for v in groups.values())
        assert all(r in ids[offs[r]:offs[r + 1]].tolist() for r in range(B)) and max(len(v) for v in groups.values()) > 1
        # every row has a candidate with another id, and some group has more than one row
        assert all(any(x != y for y in rc["idx"]) for x in rc["idx"]) and len(set(rc["idx"])) < B
    with pytest.raises(AssertionError, match="no candidate"):
        retrieval_negatives([4, 4, 4], 1)
    assert retrieval_negatives([3, 5, 5, 9, 3], 7) == retrieval_negatives([3, 5, 5, 9, 3], 7)


def test_ground_truth_csr_from_ragged_tables(mr):
    offs, ids = mr.ground_truth_csr(EVAL_IMG2TXT, 6)
    assert offs.dtype == torch.int32 and ids.dtype == torch.int32
    assert offs.tolist() == [0, 2, 3, 6, 6, 8, 10] and ids.tolist() == list(range(10))            # image 3 has no caption
    offs, ids = mr.ground_truth_csr(EVAL_TXT2IMG, 10)
    assert offs.tolist() == list(range(11)) and ids.tolist() == EVAL_TXT2IMG
    offs, ids = mr.ground_truth_csr([[2, 0], [], [1]], 3)                                         # a list of lists, order kept
    assert offs.tolist() == [0, 2, 2, 3] and ids.tolist() == [2, 0, 1]
    offs, ids = mr.ground_truth_csr({1: [4]}, 3)                                                  # queries missing from a dict: no ground truth
    assert offs.tolist() == [0, 0, 1, 1] and ids.tolist() == [4]
    offs, ids = mr.ground_truth_csr({}, 2)
    assert offs.tolist() == [0, 0, 0] and ids.numel() == 0 and ids.dtype == torch.int32
    assert mr.RECALL_KEYS == ("txt_r1", "txt_r5", "txt_r10", "txt_r_mean", "img_r1", "img_r5", "img_r10", "img_r_mean", "r_mean")


def test_host_restatement_of_the_rank_rule():
    s = np.array([[0.5, 0.9, 0.1, 0.9], [1.0, 1.0, 1.0, 1.0], [-100.0, 3.0, -100.0, -100.0]])
    assert ranks_float64(s, [[2], [1], [0]]).tolist() == [3, 0, 1]            # strictly greater: a tie does not push the ground truth down
    assert ranks_float64(s, [[2, 0], [], [4, -1]]).tolist() == [2, 2 ** 31 - 1, 2 ** 31 - 1]
    assert ranks_float64(s, [[3], [0], [1]], N=3).tolist() == [2 ** 31 - 1, 0, 0]
    r = recall_from_ranks([0, 4, 9, 2 ** 31 - 1], [0, 0])
    assert r["txt_r1"] == 25.0 and r["txt_r5"] == 50.0 and r["txt_r10"] == 75.0 and r["img_r1"] == 100.0
    assert r["r_mean"] == ((25.0 + 50.0 + 75.0) / 3 + 100.0) / 2 and list(r) == list(importlib.import_module("x2-vlm_amd.model_retrieval").RECALL_KEYS)


def test_host_tensors_are_refused(mr, synthetic, tmp_path):
    ops = importlib.import_module("x2-vlm_amd.ops")
    with pytest.raises(NotImplementedError, match="HIP path"):
        ops.itc_soft(torch.zeros(4, 4), torch.arange(4))
    with pytest.raises(NotImplementedError, match="HIP path"):
        ops.retrieval_ranks(torch.zeros(2, 4), torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(NotImplementedError, match="HIP path"):
        mr.retrieval_eval(torch.zeros(6, 10), torch.zeros(10, 6), EVAL_TXT2IMG, EVAL_IMG2TXT)
    model = mr.XVLMForRetrieval(retrieval_config("tiny", str(tmp_path)))
    b = retrieval_batch(synthetic, "tiny")
    for idx in (None, b["idx"]):
        with pytest.raises(NotImplementedError, match="HIP path"):
            model(b["image"], b["text_ids"], b["text_atts"], idx=idx)
    with pytest.raises(NotImplementedError, match="HIP path"):
        mr.retrieval_evaluation(model, [b["image"]], b["text_ids"], b["text_atts"], 2)


def test_fixture_keys():
    for name, rc in RETRIEVAL_CASES.items():
        path = "%s/%s_retrieval_step.npz" % (GOLD_DIR, name)
        assert os.path.getsize(path) < 1 << 20
        g = np.load(path)
        B, E = rc["batch"], CASES[rc["case"]]["embed_dim"]
        for k in ("loss_itc", "loss_itm", "total_grad_norm", "image_feat", "text_feat", "idx", "neg_idx"):
            assert k in g.files, (name, k)
        assert g["image_feat"].shape == (B, E) and g["text_feat"].shape == (B, E) and g["neg_idx"].shape == (2, B)
        assert g["idx"].tolist() == rc["idx"]
        assert np.allclose(np.linalg.norm(g["image_feat"], axis=1), 1.0, atol=1e-5)
        for row in range(B):
            assert all(rc["idx"][int(j)] != rc["idx"][row] for j in g["neg_idx"][:, row])
        norms = [k for k in g.files if k.startswith("gradnorm/")]
        assert "gradnorm/temp" in norms and "gradnorm/itm_head.3.weight" in norms and len(norms) > 40
        assert abs(sum(float(g[k]) ** 2 for k in norms) ** 0.5 - float(g["total_grad_norm"])) <= 1e-9 * float(g["total_grad_norm"])
        assert not any(k.startswith("gradsample/") for k in g.files)
        assert float(g["loss_itc"]) > 0 and float(g["loss_itm"]) > 0
        if rc["case"] == "tiny_video":
            assert "gradnorm/absolute_frame_pos_embed" in norms
    g = np.load("%s/tiny_retrieval_step.npz" % GOLD_DIR)
    assert float(g["eval_min_gap"]) > 0.0                                     # no exact tie among the reference's ITM scores
    t = np.load("%s/tiny_retrieval.npz" % GOLD_DIR)
    want = recall_from_ranks(ranks_float64(t["score_i2t"], [EVAL_IMG2TXT.get(i, []) for i in range(6)]),
                             ranks_float64(t["score_t2i"], [[j] for j in EVAL_TXT2IMG]))
    for k, v in want.items():
        assert float(g["eval_" + k]) == v, k
    # image 3 has no caption: it is in the denominator of every txt figure and in none of the counts
    assert want["txt_r10"] <= 100.0 * 5 / 6 + 1e-12
