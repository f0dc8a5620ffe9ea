"""Load / wait census of the row kernels from a gfx950 assembly listing of csrc/rowwise.hip
(hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only rowwise.hip -o rowwise.s).

For every kernel whose demangled name contains one of the patterns: vector memory loads (global_load_* / flat_load_* / buffer_load_*),
flat_* accesses, `s_waitcnt vmcnt(..)` instructions in the whole kernel, and for the hottest loop (the innermost-looking backward branch target
range that holds the most loads) the loads issued ahead of its first vmcnt wait.  The rule the LayerNorm section of rowwise.hip states - all
loads of a row before the first consuming instruction - reads here as `first wait after N loads` with N = every load of the loop.

usage: python probes/isa_loads_waits.py rowwise.s [pattern ...]"""
import re
import subprocess
import sys

DEFAULT = ["layernorm_bwd_kernel", "layernorm_fwd_rows_kernel", "reduce_partials", "colsum_bf16_kernel", "gemm_tn256_reduce_kernel",
           "layerscale_finish_kernel"]
LOAD = re.compile(r"^\s+(global_load|flat_load|buffer_load)_")
FLAT = re.compile(r"^\s+flat_(load|store|atomic)_")
WAIT = re.compile(r"^\s+s_waitcnt\b.*vmcnt\(")
LABEL = re.compile(r"^(\.LBB\d+_\d+):")
BRANCH = re.compile(r"^\s+s_c?branch\w*\s+(\.LBB\d+_\d+)")


def demangle(names):
    out = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    """{mangled name: body lines} for every .amdhsa kernel function of the listing"""
    cur, body, found = None, [], {}
    for line in open(path):
        m = re.match(r"^(_Z\w+|\w+):\s*(;.*)?$", line)
        if m and not line.startswith(".L"):
            cur, body = m.group(1), []
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                found[cur] = body
                cur = None
            else:
                body.append(line.rstrip("\n"))
    return found


def loops(body):
    """(start, end) line ranges of backward branches"""
    at = {m.group(1): i for i, l in enumerate(body) for m in [LABEL.match(l)] if m}
    out = []
    for i, l in enumerate(body):
        m = BRANCH.match(l)
        if m and m.group(1) in at and at[m.group(1)] < i:
            out.append((at[m.group(1)], i))
    return out


def census(body):
    nload = sum(1 for l in body if LOAD.match(l))
    nflat = sum(1 for l in body if FLAT.match(l))
    nwait = sum(1 for l in body if WAIT.match(l))
    best = None
    for a, b in loops(body):
        seg = body[a:b + 1]
        n = sum(1 for l in seg if LOAD.match(l))
        if n and (best is None or n > best[0]):
            first = 0
            for l in seg:
                if WAIT.match(l):
                    break
                first += 1 if LOAD.match(l) else 0
            best = (n, sum(1 for l in seg if WAIT.match(l)), first)
    return nload, nflat, nwait, best


def main():
    path, pats = sys.argv[1], sys.argv[2:] or DEFAULT
    ks = kernels(path)
    names = demangle(list(ks))
    print("%-72s %6s %6s %6s   %s" % ("kernel", "loads", "flat", "vmcnt", "largest loop: loads / vmcnt waits / loads ahead of the first wait"))
    for mangled in sorted(ks, key=lambda n: names[n]):
        nm = names[mangled]
        if not any(p in nm for p in pats):
            continue
        nload, nflat, nwait, best = census(ks[mangled])
        short = re.sub(r"^void ", "", nm).split("(")[0]
        print("%-72s %6d %6d %6d   %s" % (short, nload, nflat, nwait, "-" if best is None else "%d / %d / %d" % best))


if __name__ == "__main__":
    main()
