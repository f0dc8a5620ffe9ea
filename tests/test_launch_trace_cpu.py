"""Launch traces of the text paths, pinned on the CPU: kernels.call - the one choke point of every launch - is replaced by a recorder, and the
model code runs on plain CPU tensors without the library.  Per call the recorder keeps the entry-point name and every argument, classified by
its declared type in _lib._SIGS: scalars by value (floats to 6 significant digits), pointers as "null" / "ptr", an AttnArgs block as the dict
of its fields under the same rule, ctypes arrays by length.  Every scenario's trace must equal tests/golden/launch_trace.json exactly: the
sequence of entry points a path calls and their scalar arguments are part of its contract (the decode step restates the training layer's
launches, and the MLM loss, the per-sequence LM loss, the decode step and VQA ranking run the same LM-head transform and - the two losses -
the same head backward: a change to one of them that the others do not follow shows up here).

The fixture is written by `python tests/test_launch_trace_cpu.py --write`; regenerating it after a change of the traced code proves nothing -
it is regenerated only when a launch sequence is MEANT to change, and the diff of the fixture is then the review's subject.

Geometry: a 2-layer text encoder with one fusion layer, hidden size 128 (2 heads), intermediate size 256, vocabulary 100 (no multiple of
64: the padded-bias branch of the head runs), encoder width 192."""
import ctypes
import importlib
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
FIXTURE = os.path.join(ROOT, "tests", "golden", "launch_trace.json")

SELF_ATTN = ("x2_attn_fwd", "x2_attn_fwd_mask2d", "x2_attn_decode")


def _mods():
    names = ("_lib", "kernels", "engine", "xbert", "decode")
    return SimpleNamespace(**{n.strip("_"): importlib.import_module("x2-vlm_amd." + n) for n in names})


# ----------------------------------------------------------------------------- the recorder

def _value(arg, ctype, lib):
    if isinstance(arg, ctypes.Array):
        return {"len": len(arg)}
    if ctype is ctypes.POINTER(lib.AttnArgs):
        block = arg._obj
        return {name: _value(getattr(block, name), ftype, lib) for name, ftype in lib.AttnArgs._fields_}
    if ctype in (ctypes.c_float, ctypes.c_double):
        return float("%.6g" % arg)
    if ctype in (ctypes.c_int, ctypes.c_long, ctypes.c_uint):
        return int(arg)
    return "null" if arg is None or (isinstance(arg, int) and arg == 0) else "ptr"


class Recorder:
    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __call__(self, name, *args):
        sig = self.lib._SIGS[name]
        assert len(args) + 1 == len(sig), "%s: %d arguments for %d declared (the last is the stream)" % (name, len(args), len(sig))
        self.calls.append([name, [_value(a, t, self.lib) for a, t in zip(args, sig)]])

    def take(self):
        out, self.calls = self.calls, []
        return out


# ----------------------------------------------------------------------------- the scenarios

V, HD, HEADS, FF, WIDTH, L, T = 100, 128, 2, 256, 192, 8, 5


def _config(m, layers=2, fusion_layer=1, width=WIDTH):
    cfg = m.xbert.BertConfig(vocab_size=V, hidden_size=HD, num_hidden_layers=layers, num_attention_heads=HEADS, intermediate_size=FF,
                             max_position_embeddings=32)
    cfg.fusion_layer, cfg.encoder_width = fusion_layer, width
    return cfg


def _ids(rows, cols, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(4, V, (rows, cols), generator=g)


def _head_params(model):
    """(eps, dense weight, dense bias, LayerNorm weight, LayerNorm bias, decoder bias, tied word embeddings) of a model's LM head"""
    pr = model.cls.predictions
    return (model.config.layer_norm_eps, pr.transform.dense.weight, pr.transform.dense.bias, pr.transform.LayerNorm.weight,
            pr.transform.LayerNorm.bias, pr.bias, model.bert.embeddings.word_embeddings.weight)


def _scenarios(m, rec):
    """name -> trace, in a fixed order; every scenario starts from an empty WeightBank, so its weight casts are part of its trace."""
    out = {}

    def scenario(name, fn, fresh_bank=True):
        if fresh_bank:
            m.engine.BANK.invalidate()
        rec.take()
        fn()
        out[name] = rec.take()

    cfg = _config(m)
    enc2 = torch.randn(2, T, WIDTH, generator=torch.Generator().manual_seed(1))
    enc4 = torch.randn(4, T, WIDTH, generator=torch.Generator().manual_seed(2))
    ids = _ids(4, L, 3)
    atts = torch.ones(4, L, dtype=torch.long)
    atts[1, 6:] = 0
    enc_atts = torch.ones(4, T, dtype=torch.long)

    # 1. train mode: dropout at all five sites (and the embeddings'), 4 rows sharing 2 images through kv_idx
    bert = m.xbert.BertModel(cfg).train()

    def train_shared():
        m.xbert._FIXED_SEEDS.extend([1234, 5678])
        bert(ids, attention_mask=atts, encoder_hidden_states=enc2, encoder_attention_mask=enc_atts, kv_idx=torch.tensor([0, 0, 1, 1]))
        assert not m.xbert._FIXED_SEEDS
    scenario("bert_train_shared_kv", train_shared)

    # 2. eval mode, [S, L, L] tril mask, explicit position ids, one image per row: mask2d self-attention, identity cross-attention
    bert.eval()
    tril = torch.tril(torch.ones(L, L, dtype=torch.long)).expand(4, L, L)
    pids = torch.arange(L).expand(4, L)
    with torch.no_grad():
        scenario("bert_eval_mask2d", lambda: bert(ids, attention_mask=tril, position_ids=pids, encoder_hidden_states=enc4,
                                                  encoder_attention_mask=enc_atts))
        # 3. the layer ranges
        scenario("bert_mode_text", lambda: bert(ids, attention_mask=atts, mode="text"))
        hidden = torch.randn(4, L, HD, generator=torch.Generator().manual_seed(4))
        scenario("bert_mode_fusion", lambda: bert(encoder_embeds=hidden, attention_mask=atts, encoder_hidden_states=enc4,
                                                  encoder_attention_mask=enc_atts, mode="fusion"))

    # 4. the MLM head with its losses
    te = m.xbert.BertForMaskedLM(cfg).eval()
    seq = torch.randn(2, L, HD, generator=torch.Generator().manual_seed(5))
    masked_pos = torch.tensor([[1, 3, 5], [2, 4, 0]])
    labels = torch.tensor([7, 9, -100, 11, 13, -100])
    weights = torch.tensor([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0]])
    scenario("mlm_loss", lambda: te.mlm_loss_from_hidden(seq, masked_pos, labels))
    scenario("mlm_loss_keep_logits", lambda: te.mlm_loss_from_hidden(seq, masked_pos, labels, keep_logits=True))
    scenario("mlm_loss_smoothed", lambda: te.smoothed_mlm_loss_from_hidden(seq, masked_pos, labels.clamp(min=1), weights, 1, 0.1))

    # 5. the answer decoder's head on 6 rows
    dec = m.xbert.BertLMHeadModel(_config(m, layers=1, fusion_layer=0, width=HD)).eval()
    rows = torch.randn(6, HD, generator=torch.Generator().manual_seed(6)).to(torch.bfloat16)
    with torch.no_grad():
        scenario("lm_head_logits", lambda: dec.head_logits(rows))
        scenario("lm_head_loss_rows", lambda: dec.head_loss_rows(rows, labels))

    # 6. the decode stack, 2 images x 2 beams: ONE scenario (the bank is emptied in front of the construction only, as in a generate() call),
    #    recorded in its four parts
    Bi, beams, prompt = 2, 2, 2
    S = Bi * beams
    box = {}
    with torch.no_grad():
        scenario("decode_construct", lambda: box.update(stack=m.decode._TextStack(SimpleNamespace(text_encoder=te), enc2, S, beams, 16)))
        stack = box["stack"]
        scenario("decode_first_step", lambda: stack.step(_ids(Bi, prompt + 1, 7), torch.arange(prompt + 1).expand(Bi, prompt + 1).contiguous(), 0),
                 fresh_bank=False)
        scenario("decode_reorder", lambda: stack.reorder(torch.tensor([0, 0, 1, 1], dtype=torch.int32), prompt), fresh_bank=False)
        scenario("decode_later_step", lambda: stack.step(_ids(S, 2, 8), torch.arange(prompt, prompt + 2).expand(S, 2).contiguous(), prompt),
                 fresh_bank=False)

    # 7. scenario 2 with the second stream of the fusion stack switched on (on the CPU SideStream.launch runs in line): every fusion layer's
    #    K/V projection ahead of the layers instead of behind the layer's query GEMM
    def aux_ahead():
        m.engine.AUX.enabled = True
        try:
            bert(ids, attention_mask=tril, position_ids=pids, encoder_hidden_states=enc4, encoder_attention_mask=enc_atts)
        finally:
            m.engine.AUX.enabled = False
    with torch.no_grad():
        scenario("bert_eval_mask2d_aux_ahead", aux_ahead)

    # 8. the backward passes of the two LM losses and of the MLP heads: `name` (None: not kept, an earlier scenario holds it) is the forward
    #    from an emptied bank, `name_backward` (or `backward`) what scalar_of(its result).backward() launches behind it
    def with_backward(name, fn, scalar_of, backward=None):
        m.engine.BANK.invalidate()
        rec.take()
        res = fn()
        fwd = rec.take()
        if name is not None:
            out[name] = fwd
        scalar_of(res).backward()
        out[backward or name + "_backward"] = rec.take()

    word = te.bert.embeddings.word_embeddings.weight
    seq_g = seq.clone().requires_grad_()
    with_backward(None, lambda: te.mlm_loss_from_hidden(seq_g, masked_pos, labels), lambda r: r[0], backward="mlm_loss_backward")
    assert seq_g.grad is not None and word.grad is not None
    with_backward(None, lambda: te.smoothed_mlm_loss_from_hidden(seq_g, masked_pos, labels.clamp(min=1), weights, 1, 0.1), lambda r: r[0],
                  backward="mlm_loss_smoothed_backward")

    # ... with the word-embedding gradient parked for the embedding backward instead of returned (the segmented step's route)
    word.grad = None
    with pytest.MonkeyPatch.context() as tie:
        tie.setattr(m.engine, "TIE_WORD_GRAD", True)
        try:
            with_backward(None, lambda: te.mlm_loss_from_hidden(seq_g, masked_pos, labels), lambda r: r[0], backward="mlm_loss_backward_tied")
            assert len(m.engine._TIED_DWORD) == 1 and word.grad is None
        finally:
            m.engine._TIED_DWORD.clear()

    # 9. the per-sequence LM loss of the answer decoder: the 6 rows as 2 sequences of 3 scored positions
    head = _head_params(dec)
    rows_g = rows.float().requires_grad_()
    c = torch.tensor([0.5, 0.25])
    with_backward("lm_seq_loss", lambda: m.engine.SeqLmLossFn.apply(rows_g, labels, 3, c, *head), lambda r: r[1])
    with_backward(None, lambda: m.engine.SeqLmLossFn.apply(rows_g, labels, 3, None, *head), lambda r: r[0].sum(),
                  backward="lm_seq_loss_unweighted_backward")

    # 10. a build_mlp head on 4 rows: input width 128 takes the bf16 MFMA first layer, 100 (no multiple of 64) the fp32 one
    ops, xvlm = importlib.import_module("x2-vlm_amd.ops"), importlib.import_module("x2-vlm_amd.xvlm")
    for kind, width in (("mfma", 128), ("f32", 100)):
        mlp = xvlm.build_mlp(width, 2)
        x = torch.randn(4, width, generator=torch.Generator().manual_seed(9)).requires_grad_()
        with_backward("mlp_head_" + kind, lambda: ops.mlp_head(mlp, x), lambda y: y.sum())
        with torch.no_grad():
            scenario("head_first_linear_" + kind, lambda: ops.head_first_linear(mlp, x))
    return out


def record_all():
    """Every scenario, recorded from the code as it stands: kernels.call replaced by the recorder, and kernels.raw_stream - workspace() asks
    it, and the real one initialises the GPU - by a constant."""
    m = _mods()
    rec = Recorder(m.lib)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(m.kernels, "call", rec)
        mp.setattr(m.kernels, "raw_stream", lambda: 0)
        return _scenarios(m, rec)


# ----------------------------------------------------------------------------- the tests

@pytest.fixture(scope="module")
def recorded():
    return record_all()


def test_every_launch_trace_equals_the_fixture(recorded):
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(recorded) == sorted(want)
    for name in want:
        assert [c[0] for c in recorded[name]] == [c[0] for c in want[name]], "%s: another sequence of entry points" % name
        for i, (g, w) in enumerate(zip(recorded[name], want[name])):
            assert g == w, "%s: call %d (%s) has other arguments" % (name, i, w[0])
    assert recorded == want


def _layers(names):
    """The per-layer name sequences of a trace: a layer starts at the QKV GEMM (the first GEMM directly in front of a self-attention launch)
    and ends behind the LayerNorm that follows its two FFN GEMMs."""
    start = next(i for i in range(len(names) - 1) if names[i] == "x2_gemm_nt" and names[i + 1] in SELF_ATTN)
    layers, cur = [], []
    for n in names[start:]:
        cur.append(n)
        if cur[-3:] == ["x2_gemm_nt", "x2_gemm_nt", "x2_layernorm_fwd"]:
            layers.append(cur)
            cur = []
    return layers, cur


def test_decode_layers_launch_what_the_training_layers_launch(recorded):
    """Per layer the decode step runs the training forward's entry points with x2_attn_decode in place of the self-attention x2_attn_fwd.  The one
    launch a decode step's fusion layer does not repeat is the K/V projection of the image tokens (the GEMM between the query GEMM and the
    cross-attention): _TextStack projects it once, at construction."""
    want = recorded
    train, rest = _layers([c[0] for c in want["bert_train_shared_kv"]])
    assert len(train) == 2 and rest == []
    text = ["x2_gemm_nt", "x2_attn_fwd", "x2_gemm_nt", "x2_layernorm_fwd", "x2_gemm_nt", "x2_gemm_nt", "x2_layernorm_fwd"]
    assert train[0] == text
    assert train[1] == text[:4] + ["x2_gemm_nt", "x2_gemm_nt", "x2_attn_fwd", "x2_gemm_nt", "x2_layernorm_fwd"] + text[4:]
    expect = [[n if i != 1 else "x2_attn_decode" for i, n in enumerate(layer)] for layer in train]
    del expect[1][5]                                                          # the K/V projection
    assert [c[0] for c in want["decode_construct"]].count("x2_gemm_nt") == 1   # ... of the one fusion layer, ahead of the steps
    for step in ("decode_first_step", "decode_later_step"):
        got, tail = _layers([c[0] for c in want[step]])
        assert got == expect, step
        assert tail[0] == "x2_gather_rows"                                     # then the head on the [MASK] rows


def test_second_stream_projects_the_same_kv_ahead_of_the_layers(recorded):
    """engine.AUX on: the launches of the in-line pass, with each fusion layer's K/V GEMM (same arguments) moved in front of the first layer."""
    inline, ahead = recorded["bert_eval_mask2d"], recorded["bert_eval_mask2d_aux_ahead"]
    names = [c[0] for c in inline]
    kv = [i for i in range(2, len(names)) if names[i - 1:i + 2] == ["x2_gemm_nt", "x2_gemm_nt", "x2_attn_fwd"]]
    assert len(kv) == 1                                                        # one fusion layer
    first = next(i for i in range(len(names) - 1) if names[i] == "x2_gemm_nt" and names[i + 1] in SELF_ATTN)
    moved = list(inline)
    moved.insert(first, moved.pop(kv[0]))
    assert ahead == moved


LM_HEAD_BACKWARD = ["x2_colsum_bf16", "x2_gemm_nt_splitk", "x2_layernorm_bwd", "x2_gelu_f32", "x2_cast_bf16", "x2_colsum_bf16", "x2_gemm_nt",
                    "x2_gemm_tn_grouped"]


def test_the_two_lm_losses_share_the_head(recorded):
    """MlmLossFn and SeqLmLossFn differ in the loss only: in front of the fused decoder GEMM both run one transform (dense + GELU, LayerNorm,
    the casts of the tied decoder), behind the kernel that writes the logit gradient both run one backward - call for call with the same
    arguments, the two scenarios having 6 rows each.  The MLM loss alone gathers its rows, so its backward alone ends with their scatter."""
    mlm, seq = recorded["mlm_loss"], recorded["lm_seq_loss"]
    first = [c[0] for c in mlm].index("x2_cast_bf16")
    assert [c[0] for c in mlm[:first]] == ["x2_gather_rows"]
    assert seq[:-2] == mlm[first:-2]
    assert seq[-2] == mlm[-2] and seq[-2][0] == "x2_mlm_ce_fwd"                # stage 1 of both losses; the combine launches differ
    assert [seq[-1][0], mlm[-1][0]] == ["x2_seq_loss_combine", "x2_ce_combine"]
    mlm_b, seq_b = recorded["mlm_loss_backward"], recorded["lm_seq_loss_backward"]
    assert [c[0] for c in mlm_b] == ["x2_mlm_ce_bwd"] + LM_HEAD_BACKWARD + ["x2_scatter_rows"]
    assert [c[0] for c in seq_b] == ["x2_mlm_seq_bwd"] + LM_HEAD_BACKWARD
    assert seq_b[1:] == mlm_b[1:-1]
    for other, first_call in (("mlm_loss_smoothed_backward", "x2_mlm_ls_bwd"), ("lm_seq_loss_unweighted_backward", "x2_mlm_seq_bwd")):
        assert recorded[other][0][0] == first_call and recorded[other][1:len(seq_b)] == seq_b[1:], other


def test_parking_the_word_gradient_launches_nothing_else(recorded):
    """engine.TIE_WORD_GRAD only changes where the tied decoder's gradient goes (the scenario asserts that it is parked in engine._TIED_DWORD
    and that the word embeddings receive none)"""
    assert recorded["mlm_loss_backward_tied"] == recorded["mlm_loss_backward"]


@pytest.mark.parametrize("kind", ["mfma", "f32"])
def test_head_first_linear_is_how_mlp_head_starts(recorded, kind):
    first, whole = recorded["head_first_linear_" + kind], recorded["mlp_head_" + kind]
    assert first[-1][0] == ("x2_gemm_nt" if kind == "mfma" else "x2_linear_f32")
    assert 0 < len(first) < len(whole) and whole[:len(first)] == first


def _dump(traces, path):
    with open(path, "w") as f:
        f.write("{\n")
        for si, (name, calls) in enumerate(traces.items()):
            f.write(" %s: [\n" % json.dumps(name))
            f.write(",\n".join("  " + json.dumps(c, separators=(",", ":")) for c in calls))
            f.write("\n ]%s\n" % ("," if si + 1 < len(traces) else ""))
        f.write("}\n")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_launch_trace_cpu.py --write    (rewrites tests/golden/launch_trace.json)")
    _dump(record_all(), FIXTURE)
    print("wrote", FIXTURE)
