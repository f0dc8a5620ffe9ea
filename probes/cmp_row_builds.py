"""A/B of two builds of the row kernels (X2VLM_HIP_LIB picks the library; run once per library, alternating): bits and per-launch time of the
LayerNorm backward and the stage-2 reducer at the training step's own shapes.  GPU box only.

  python probes/cmp_row_builds.py --dump DIR --json FILE     run the launches on seeded inputs, write every output and workspace to DIR/*.npy,
                                                             time each launch and write {name: us} to FILE
  python probes/cmp_row_builds.py --same DIR_A DIR_B         exit 0 iff the two dumps are equal as integers, file by file
  python probes/cmp_row_builds.py --table A.json,A2.json,.. B.json,B2.json,..     min over the runs of each side, us and TB/s, side by side

Launches: LayerNorm backward 12608 x 768 (post = 1: layernorm_bwd_kernel<3, 2>; bf16 dy + dres: <3, 1>), 7680 x 768 and 3840 x 768 (fp32 dy, dcol: <3, 0>),
18464 x 1024 (post = 1: <4, 2>), every one with defer = 1 so that stage 2 is timed on its own; one x2_reduce_partials_multi over 12 descriptors
built from those workspaces; layernorm_fwd at 12608 x 768 (layernorm_fwd_rows_kernel<3, 2>) as the reachable rate of the same box.
Timing: each launch runs over 8 rotating buffer sets (nothing stays cache-resident), 5 passes over the sets per round, the minimum of 3 rounds
that interleave all the launches."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

NSETS, PASSES, ROUNDS = 8, 5, 3
# name -> (rows, D, mode, bytes per element)
LNB = {"lnb_12608x768_post": (12608, 768, 2, 16), "lnb_12608x768_bf16": (12608, 768, 1, 14), "lnb_7680x768_f32_dcol": (7680, 768, 0, 14),
       "lnb_3840x768_f32_dcol": (3840, 768, 0, 14), "lnb_18464x1024_post": (18464, 1024, 2, 16)}
RED12 = ["lnb_12608x768_post", "lnb_12608x768_bf16", "lnb_7680x768_f32_dcol", "lnb_3840x768_f32_dcol"] * 3


def same(a, b):
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and names, "different file lists"
    bad = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        eq = x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
        bad += 0 if eq else 1
        print("%-44s %s" % (n, "identical" if eq else "DIFFERENT"))
    print("%d files, %d differ" % (len(names), bad))
    return bad == 0


def table(a_files, b_files):
    def best(files):
        runs = [json.load(open(f)) for f in files]
        return {k: min(r[k]["us"] for r in runs) for k in runs[0]}, runs[0]
    (a, meta), (b, _) = best(a_files), best(b_files)
    print("%-26s %9s %9s %9s   %8s %8s   (MB per launch = byte floor)" % ("launch", "MB", "A us", "B us", "A TB/s", "B TB/s"))
    for k in a:
        mb = meta[k]["mb"]
        print("%-26s %9.1f %9.1f %9.1f   %8.2f %8.2f" % (k, mb, a[k], b[k], mb / a[k], mb / b[k]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump")
    ap.add_argument("--json")
    ap.add_argument("--same", nargs=2)
    ap.add_argument("--table", nargs=2)
    args = ap.parse_args()
    if args.same:
        sys.exit(0 if same(*args.same) else 1)
    if args.table:
        return table(args.table[0].split(","), args.table[1].split(","))

    import torch
    K = importlib.import_module("x2-vlm_amd.kernels")
    dev = "cuda"
    gen = torch.Generator(device=dev).manual_seed(1234)

    def rnd(*shape, dtype=torch.float32):
        return torch.randn(*shape, generator=gen, device=dev).to(dtype)

    class Lnb:
        def __init__(self, rows, D, mode):
            self.rows, self.D, self.mode, self.nblk = rows, D, mode, (rows + 15) // 16
            self.w = rnd(D) * 0.1 + 1
            self.sets = []
            for _ in range(NSETS):
                x = rnd(rows, D) * 2 + 0.5
                _, _, mean, rstd = K.layernorm_fwd(x, self.w, self.w, 1e-6, want_bf16=False)
                s = dict(x=x, mean=mean, rstd=rstd, dy=rnd(rows, D, dtype=torch.bfloat16 if mode else torch.float32),
                         dres=rnd(rows, D) if mode else None, dx=torch.empty(rows, D, device=dev),
                         dxb=None if mode == 1 else torch.empty(rows, D, device=dev, dtype=torch.bfloat16),
                         prs=(torch.rand(rows, generator=gen, device=dev) > 0.1).float() * 1.1 if mode == 2 else None,
                         ws=torch.empty(self.nblk * 3 * D, device=dev), outs=[torch.zeros(D, device=dev) for _ in range(3)])
                self.sets.append(s)

        def launch(self, i):
            s = self.sets[i % NSETS]
            o = s["outs"]
            K.call("x2_layernorm_bwd", K.ptr(s["dy"]), 1 if self.mode else 0, K.ptr(s["x"]), K.ptr(s["mean"]), K.ptr(s["rstd"]), K.ptr(self.w), K.ptr(s["dres"]),
                   K.ptr(s["dx"]), K.ptr(s["dxb"]), K.ptr(o[0]), K.ptr(o[1]), None if self.mode == 1 else K.ptr(o[2]), self.rows, self.D, 0, 0, 0, 1.0, 0, 0, 1.0, None,
                   K.ptr(s["ws"]), 1, 1 if self.mode == 2 else 0, K.ptr(s["prs"]))

    lnb = {k: Lnb(r, D, m) for k, (r, D, m, _) in LNB.items()}

    def red_desc(i):
        flat = []
        for j, k in enumerate(RED12):
            L = lnb[k]
            s = L.sets[(i + j // 4) % NSETS]
            o = red_outs[i % NSETS][j]
            flat += [s["ws"].data_ptr(), L.nblk, 3, L.D, o[0].data_ptr(), o[1].data_ptr(), 0 if L.mode == 1 else o[2].data_ptr(), 0]
        return (C.c_int64 * len(flat))(*flat)

    red_outs = [[[torch.zeros(lnb[k].D, device=dev) for _ in range(3)] for k in RED12] for _ in range(NSETS)]
    xf = [rnd(12608, 768) for _ in range(NSETS)]
    wf = rnd(768)

    for L in lnb.values():                      # every workspace written once before the reducer reads it
        for i in range(NSETS):
            L.launch(i)
    torch.cuda.synchronize()
    descs = [red_desc(i) for i in range(NSETS)]
    launches = {k: L.launch for k, L in lnb.items()}
    launches["reduce_multi_12desc"] = lambda i: K.call("x2_reduce_partials_multi", descs[i % NSETS], len(RED12))
    yb, mu, rsd = torch.empty(12608, 768, device=dev, dtype=torch.bfloat16), torch.empty(12608, device=dev), torch.empty(12608, device=dev)
    launches["lnf_rows_12608x768"] = lambda i: K.call("x2_layernorm_fwd", K.ptr(xf[i % NSETS]), K.ptr(wf), K.ptr(wf), K.ptr(yb), None, K.ptr(mu), K.ptr(rsd),
                                                      12608, 768, 1e-6, 0, 0, 0, 1.0, None)
    mb = {k: r * D * b / 1e6 for k, (r, D, _, b) in LNB.items()}
    mb["reduce_multi_12desc"] = sum(lnb[k].nblk * 3 * lnb[k].D * 4 for k in RED12) / 1e6
    mb["lnf_rows_12608x768"] = 12608 * 768 * 6 / 1e6

    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for k, L in lnb.items():
            s = L.sets[0]
            for n in ("dx", "dxb", "ws"):
                if s[n] is not None:
                    t = s[n].cpu()
                    np.save(os.path.join(args.dump, "%s.%s.npy" % (k, n)), (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy())
        launches["reduce_multi_12desc"](0)
        torch.cuda.synchronize()
        for j, k in enumerate(RED12):
            for q, o in enumerate(red_outs[0][j]):
                np.save(os.path.join(args.dump, "reduce.%02d.%s.o%d.npy" % (j, k, q)), o.cpu().numpy())

    best = {k: float("inf") for k in launches}
    for k, f in launches.items():
        f(0)
    torch.cuda.synchronize()
    for _ in range(ROUNDS):
        for k, f in launches.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(NSETS * PASSES):
                f(i)
            e.record()
            torch.cuda.synchronize()
            best[k] = min(best[k], a.elapsed_time(e) * 1e3 / (NSETS * PASSES))
    res = {k: {"us": best[k], "mb": mb[k]} for k in launches}
    for k, v in res.items():
        print("%-26s %8.1f us  %7.1f MB  %5.2f TB/s" % (k, v["us"], v["mb"], v["mb"] / v["us"]))
    if args.json:
        json.dump(res, open(args.json, "w"))


if __name__ == "__main__":
    main()
