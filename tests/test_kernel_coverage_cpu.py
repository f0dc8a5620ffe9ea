"""Name-level kernel coverage: every instantiation of the project's own HIP kernels that the committed step traces show the training
step launching (X2VLM-base, X2VLM-large, the region iteration, video) is launched by the kernel-level GPU tests as well - the
committed trace of `pytest tests/test_kernels_gpu.py tests/test_kernel_variants_gpu.py -m gpu` under rocprofv3.  Launched is not
the same as checked (branches inside a kernel, sizes, modes: the tests themselves state those), but a kernel the tests never
launch is checked only by the whole-model gates.  Re-trace (probes/prof_summary.py) and re-commit when kernels are added."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILES = os.path.join(ROOT, "profiles")
STEP_TRACES = ["r12m_base_serialized_kernel_stats.txt", "r12m_large_serialized_kernel_stats.txt",
               "r13a_region_serialized_kernel_stats.txt", "r13a_video_serialized_kernel_stats.txt"]
TEST_TRACE = "r13a_kernel_tests_kernel_stats.txt"


def project_kernels():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "x2-vlm_amd", "csrc", "*.hip")):
        with open(path) as f:
            src = f.read()
        names.update(re.findall(r"__global__[^;{}]*?\bvoid\s+(\w+)\s*\(", src))
    return names


def trace_names(name):
    """kernel column of a probes/prof_summary.py table (names as the summary prints them, long ones cut to 59 chars + '...')"""
    out = set()
    with open(os.path.join(PROFILES, name)) as f:
        for line in f:
            if line.startswith("#") or line.startswith("kernel "):
                continue
            m = re.match(r"^(.*?)\s+\d+\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+[\d.]+\s+[\d.]+\s*$", line)
            if m and m.group(1).strip():
                out.add(m.group(1).strip())
    return out


def own(names, kernels):
    return {n for n in names if re.split(r"[<.]", n)[0] in kernels}


def test_kernel_names_come_from_the_sources():
    k = project_kernels()
    for n in ("layernorm_fwd_kernel", "layernorm_fwd_rows_kernel", "layernorm_bwd_kernel", "reduce_partials_multi_kernel", "colsum_f32_kernel",
              "attn_bwd_dq_kernel", "attn_bwd_dkv_kernel", "sample_negatives_kernel", "gemm_nt_kernel"):
        assert n in k, n
    for t in STEP_TRACES + [TEST_TRACE]:
        assert len(own(trace_names(t), k)) >= 25, t


def test_every_step_instantiation_is_launched_by_the_kernel_tests():
    k = project_kernels()
    tested = own(trace_names(TEST_TRACE), k)
    missing = {}
    for t in STEP_TRACES:
        for n in sorted(own(trace_names(t), k) - tested):
            missing.setdefault(n, []).append(t)
    assert not missing, "instantiations the step launches and no kernel test does:\n" + "\n".join("  %s  (%s)" % (n, ", ".join(v))
                                                                                              for n, v in sorted(missing.items()))


def test_the_named_variants_are_in_the_kernel_tests_trace():
    tested = trace_names(TEST_TRACE)
    for n in ("layernorm_fwd_rows_kernel<3, 2>", "layernorm_fwd_rows_kernel<4, 2>", "layernorm_fwd_kernel<4>", "layernorm_fwd_kernel<8>",
              "layernorm_bwd_kernel<4, 0>", "layernorm_bwd_kernel<4, 1>", "layernorm_bwd_kernel<4, 2>", "layernorm_bwd_kernel<8, 0>",
              "colsum_f32_kernel", "sample_negatives_kernel", "reduce_partials_multi_kernel"):
        assert n in tested, n
    for pre in ("attn_bwd_dq_kernel<8, 1, false", "attn_bwd_dkv_kernel<8, 1, false"):
        assert any(n.startswith(pre) for n in tested), pre
