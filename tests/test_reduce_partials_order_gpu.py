"""The summation order of x2_reduce_partials_multi, bit for bit.

The kernel only adds fp32 numbers, so a float32 numpy emulation that adds the same numbers in the same order gives the same bits.  The order
(csrc/rowwise.hip, reduce_partials_multi_kernel) for one output column and nblk partial rows v[0..nblk):
  * slice sl (0..63) walks b = sl, sl + 64, ...; while b + 192 < nblk it adds (v[b] + v[b+64]) + (v[b+128] + v[b+192]) to its sum and
    moves on by 256; then it adds the remaining rows one by one;
  * slice 0's sum takes the sums of slices 1..63 in that order (slices without rows add +0.0);
  * out = out + total.
A width that is no multiple of 4 takes the scalar path: every slice adds its rows one by one, the rest is the same.
Each case also holds the device result to 1e-5 of the float64 sum's max-abs (`relerr`), the bound tests/test_kernel_extents_gpu.py uses for
this kernel.  The emulation itself is held to float64 on the CPU (test_emulation_matches_float64_cpu), so the order is pinned without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from kernel_helpers import K, relerr  # noqa: F401 (fixture)

NBLK = [1, 3, 63, 64, 65, 255, 256, 257, 300, 788]
NK = [1, 3, 4]
WIDTH = [4, 20, 768, 770]
f32 = np.float32


def emulate(part, init):
    """part [nblk][width] float32, init [width] float32 -> init + sum over rows in the kernel's order, float32 throughout"""
    nblk, width = part.shape
    vec = width % 4 == 0
    sums = np.zeros((64, width), dtype=f32)
    for sl in range(64):
        s = np.zeros(width, dtype=f32)
        b = sl
        if vec:
            while b + 192 < nblk:
                s = s + ((part[b] + part[b + 64]) + (part[b + 128] + part[b + 192]))
                b += 256
        while b < nblk:
            s = s + part[b]
            b += 64
        sums[sl] = s
    total = sums[0]
    for sl in range(1, 64):
        total = total + sums[sl]
    return init + total


_PARTS = {}


def case(nblk, nk, width):
    """(partials [nblk][nk][width], initial outputs [nk][width]) as float32 numpy, seeded by the shape; values of mixed sign and magnitude so
    that another order rounds differently"""
    key = (nblk, nk, width)
    if key not in _PARTS:
        rng = np.random.default_rng(nblk * 10007 + nk * 101 + width)
        part = (rng.standard_normal((nblk, nk, width)) * np.exp(rng.standard_normal((nblk, nk, width)))).astype(f32)
        init = (rng.standard_normal((nk, width)) * 3.0 + 0.5).astype(f32)
        _PARTS[key] = (part, init)
    return _PARTS[key]


def expected(part, init, null=()):
    return [None if k in null else emulate(np.ascontiguousarray(part[:, k]), init[k]) for k in range(part.shape[1])]


def as_int(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("width", WIDTH)
@pytest.mark.parametrize("nblk", NBLK)
def test_emulation_matches_float64_cpu(nblk, width):
    """the emulation is a sum.  Every element of the result is reached through at most ceil(nblk / 64) + 64 fp32 additions (a slice's quads and
    singles, 63 slice sums, the output), so it differs from float64 by at most that many half-ulps of the sum of magnitudes."""
    part, init = case(nblk, 3, width)
    got = emulate(np.ascontiguousarray(part[:, 1]), init[1])
    ref = init[1].astype(np.float64) + part[:, 1].astype(np.float64).sum(0)
    scale = np.abs(init[1]).astype(np.float64) + np.abs(part[:, 1]).astype(np.float64).sum(0)
    assert float((np.abs(got - ref) / scale).max()) <= ((nblk + 63) // 64 + 64) * 2.0 ** -24
    assert relerr(torch.from_numpy(got), torch.from_numpy(ref)) < 1e-5
    if nblk == 1:
        assert np.array_equal(as_int(got), as_int(init[1] + (np.zeros(width, f32) + part[0, 1])))


def run_multi(K, cases, nulls=None):
    """one x2_reduce_partials_multi call over `cases` [(part, init)] -> per case the list of device outputs as numpy (None where the slot is null)"""
    nulls = nulls or [()] * len(cases)
    flat, keep, outs = [], [], []
    for (part, init), null in zip(cases, nulls):
        nblk, nk, width = part.shape
        pd = torch.from_numpy(part).to("cuda")
        os_ = [None if k in null else torch.from_numpy(init[k].copy()).to("cuda") for k in range(nk)]
        keep.append(pd)
        outs.append(os_)
        flat += [pd.data_ptr(), nblk, nk, width] + [0 if o is None else o.data_ptr() for o in os_] + [0] * (4 - nk)
    K.call("x2_reduce_partials_multi", (C.c_int64 * len(flat))(*flat), len(cases))
    torch.cuda.synchronize()
    return [[None if o is None else o.cpu().numpy() for o in os_] for os_ in outs]


def check(got, part, init, null=()):
    want = expected(part, init, null)
    for k, (g, w) in enumerate(zip(got, want)):
        if w is None:
            assert g is None
            continue
        assert np.array_equal(as_int(g), as_int(w)), "shape %s output %d: %d of %d elements differ from the emulated order" % (
            part.shape, k, int((as_int(g) != as_int(w)).sum()), w.size)
        ref = init[k].astype(np.float64) + part[:, k].astype(np.float64).sum(0)
        assert relerr(torch.from_numpy(g), torch.from_numpy(ref)) < 1e-5, (part.shape, k)


@pytest.mark.gpu
@pytest.mark.parametrize("nk", NK)
@pytest.mark.parametrize("nblk", NBLK)
def test_order_single_descriptor(K, nblk, nk):
    """one descriptor per call, every width (770: the scalar path), outputs pre-filled"""
    for width in WIDTH:
        part, init = case(nblk, nk, width)
        check(run_multi(K, [(part, init)])[0], part, init)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [16, 17])
def test_order_many_descriptors_mixed_shapes(K, count):
    """16 descriptors fill one launch, 17 split into two; shapes mixed inside the call; a null output in the middle of every nk >= 3 descriptor"""
    shapes = [(NBLK[i % len(NBLK)], NK[(i // 2) % len(NK)], WIDTH[(i // 3) % len(WIDTH)]) for i in range(count)]
    cases = [case(*s) for s in shapes]
    nulls = [(1,) if s[1] >= 3 else () for s in shapes]
    got = run_multi(K, cases, nulls)
    for g, (part, init), null in zip(got, cases, nulls):
        check(g, part, init, null)


@pytest.mark.gpu
def test_order_output_at_any_float(K):
    """an output that starts 4 bytes past a 16-byte boundary (a slice of a flat gradient buffer)"""
    part, init = case(300, 3, 768)
    pd = torch.from_numpy(part).to("cuda")
    flatbuf = torch.zeros(3 * 768 + 8, device="cuda")
    outs = [flatbuf[1 + k * 768:1 + (k + 1) * 768] for k in range(3)]
    for k in range(3):
        outs[k].copy_(torch.from_numpy(init[k]))
    desc = [pd.data_ptr(), 300, 3, 768] + [o.data_ptr() for o in outs] + [0]
    K.call("x2_reduce_partials_multi", (C.c_int64 * 8)(*desc), 1)
    torch.cuda.synchronize()
    check([o.cpu().numpy() for o in outs], part, init)
    assert float(flatbuf[0]) == 0.0 and float(flatbuf[1 + 3 * 768:].abs().max()) == 0.0
