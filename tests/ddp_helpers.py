"""Shared by tests/test_ddp_gpu.py and tests/test_mixed_flow_gpu.py (a plain module, not collected)."""
import torch


def _compare(got, want, what, etol=8e-2):
    total = float(torch.sqrt(sum((g.double() ** 2).sum() for g in want.values())))
    bad = []
    for name, ref in want.items():
        if name == "text_encoder.cls.predictions.decoder.weight" or name not in got:
            continue
        g = got[name].double()
        ref = ref.double()
        nerr = abs(float(g.norm()) - float(ref.norm())) / max(float(ref.norm()), 1e-2 * total)
        eerr = float((g - ref).abs().max()) / max(float(ref.abs().max()), 1e-2 * total / max(ref.numel(), 1) ** 0.5)
        if nerr > 3e-2 or eerr > etol:
            bad.append((name, nerr, eerr))
    missing = [n for n in want if n not in got and n != "text_encoder.cls.predictions.decoder.weight"
               and float(want[n].abs().max()) > 0]
    assert not missing, "%s: no gradient for %s" % (what, missing[:5])
    assert not bad, "%s: %d tensors out of tolerance, worst %s" % (what, len(bad), sorted(bad, key=lambda b: -b[2])[:5])
