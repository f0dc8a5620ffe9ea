"""Static guard on bench.py's multi-rank control flow: a training step contains collectives (ITC all-gather, gradient
all-reduce), so nothing that runs a step or a collective may sit under `if rank == 0` - rank 0 would wait for peers that
never come (this deadlocked every N > 1 run once)."""
import ast
import os

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")
FORBIDDEN = {"step", "_step", "eager_step", "fwd_bwd", "runner", "timed_gemms", "model", "fence"}


def _is_rank0_test(node):
    return (isinstance(node, ast.Compare) and isinstance(node.left, ast.Name) and node.left.id == "rank" and
            len(node.ops) == 1 and isinstance(node.ops[0], ast.Eq) and isinstance(node.comparators[0], ast.Constant) and
            node.comparators[0].value == 0)


def _calls(nodes):
    for n in nodes:
        for c in ast.walk(n):
            if isinstance(c, ast.Call):
                f = c.func
                if isinstance(f, ast.Name):
                    yield f.id, c.lineno
                elif isinstance(f, ast.Attribute) and isinstance(f.value, ast.Name):
                    yield "%s.%s" % (f.value.id, f.attr), c.lineno


def test_no_step_or_collective_under_rank0_only():
    tree = ast.parse(open(SRC).read())
    bad = []
    for node in ast.walk(tree):
        if isinstance(node, ast.If) and _is_rank0_test(node.test):
            for name, line in _calls(node.body):
                if name in FORBIDDEN or name.startswith("dist."):
                    bad.append((name, line))
    assert not bad, "rank-0-only code runs steps / collectives: %s" % bad


def test_contract_fields_present():
    src = open(SRC).read()
    for key in ('"metric"', '"value"', '"unit"', '"n_gpus"', '"steps"', '"warmup"', '"ms_per_step"', '"higher_is_better"', '"scaling"',
                '"vs_baseline"', '"dtype"', '"data"', '"config"', '"roofline"', '"cpu_baseline"', '"workload"', '"bound"', '"achieved"',
                '"peak"', '"frac"', '"traffic"', '"cores"', '"kind"', '"sample"'):
        assert key in src, key


def test_plain_and_full_options(tmp_path):
    """--full (the extra measurements) and --dump-outputs exist; dump_outputs writes float arrays, the same sample in every run."""
    import importlib.util
    import subprocess
    import sys

    import numpy as np
    import torch
    r = subprocess.run([sys.executable, SRC, "--help"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout, r.stdout + r.stderr
    spec = importlib.util.spec_from_file_location("bench_under_test", SRC)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(64, 80), torch.nn.Linear(80, 3), torch.nn.Linear(3, 3, bias=False))
    model[2].weight.requires_grad_(False)
    y = model(torch.randn(5, 64)).square().mean()
    y.backward()
    files = [bench.dump_outputs(str(tmp_path / d), {"loss_x": y.detach()}, model) for d in ("a", "b")]
    assert files[0] == files[1] == ["grad_norms.npy", "grad_sample.npy", "loss_x.npy"]
    for f in files[0]:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert np.load(tmp_path / "a" / "grad_norms.npy").shape == (len(grads),)
    assert np.load(tmp_path / "a" / "grad_sample.npy").size == sum(min(g.numel(), bench.DUMP_SAMPLE) for g in grads)
    assert float(np.load(tmp_path / "a" / "loss_x.npy")) == float(y.detach())
