"""What the kernel test files share (a plain module, not collected): seeded inputs, the error metrics, the K / lib fixtures and the pinned
kernel variants.  Every knob is pinned through _lib.tuned: a refused knob raises instead of testing the default kernel under the variant's
name, and the value that was there before comes back afterwards."""
import importlib

import pytest
import torch

tuned = importlib.import_module("x2-vlm_amd._lib").tuned
set_tune = importlib.import_module("x2-vlm_amd._lib").set_tune


@pytest.fixture(scope="module")
def K():
    return importlib.import_module("x2-vlm_amd.kernels")


@pytest.fixture(scope="module")
def lib():
    return importlib.import_module("x2-vlm_amd._lib").lib()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def bf(t):
    return t.to(torch.bfloat16)


def relerr(got, ref):
    got = got.detach().float().cpu().double()
    ref = ref.detach().double()
    assert bool(torch.isfinite(got).all()), "non-finite result"
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-12))


def slice_relerr(got, ref, floor=1e-3):
    """relerr of every slice along dim 0 (a row, a chunk, a (sequence, head) block) against that slice's own reference max-abs, floored at
    `floor` x the tensor's max-abs so that a slice of (near) zeros is held to the tensor's scale instead of dividing by ~0: a
    wrong row or head cannot hide behind a larger one elsewhere in the tensor"""
    got = got.detach().float().cpu().double().reshape(ref.shape[0], -1)
    ref = ref.detach().double().reshape(ref.shape[0], -1)
    den = ref.abs().amax(1).clamp_min(floor * float(ref.abs().max())).clamp_min(1e-30)
    return float(((got - ref).abs().amax(1) / den).max())


def rowerr(got, ref):
    """slice_relerr of a [rows, D] tensor, row by row"""
    return slice_relerr(got, ref)


# NT GEMM variants as (key 1, key 3, key 15): the 128-column tiles, the 8-wave 256-column kernel at its four heights, the ping-pong kernel
# (32x32x16 MFMAs) at 32 x value rows
NT_TILES = [(1, 1, 0), (1, 2, 0), (1, 3, 0), (1, 4, 0), (3, 8, 0), (3, 7, 0), (3, 6, 0), (3, 5, 0), (0, 0, 3), (0, 0, 4), (0, 0, 5), (0, 0, 6)]
NT_IDS = ["tile128x128", "tile192x128", "tile64x128", "tile160x128", "nt256x256", "nt224x256", "nt192x256", "nt160x256",
          "pingpong96x256", "pingpong128x256", "pingpong160x256", "pingpong192x256"]


def nt_pinned(param):
    return tuned({1: param[0], 3: param[1], 15: param[2]})


@pytest.fixture(params=NT_TILES, ids=NT_IDS)
def nt_tile(request):
    with nt_pinned(request.param):
        yield request.param


@pytest.fixture(params=NT_TILES[:4], ids=NT_IDS[:4])
def nt_tile128(request):
    with nt_pinned(request.param):
        yield request.param


@pytest.fixture(params=[1, 2], ids=["tn128x128", "tn256x256"])
def tn_tile(request):
    with tuned({5: request.param}):      # 1: always the 128x128 kernel, 2: 256x256 whenever the contraction allows
        yield request.param


dev = "cuda"
BF16, F32, I32, I64 = torch.bfloat16, torch.float32, torch.int32, torch.int64

# ------------------------------------------------------------------------------------------------ the extent guard (tests/test_kernel_extents_gpu.py; CPU-testable)
# sentinel bit patterns: NaNs with a payload for the float types (as the integer of the same width), fixed negative values for the integer types
_INT_OF = {F32: I32, BF16: torch.int16, I32: I32, I64: I64}
SENTINEL = {F32: 0x7FC5A5A5, BF16: 0x7FC5, I32: -0x5A5A5A5B, I64: -0x5A5A5A5A5A5A5A5B}
LEAD = 4096
TALLEST_TILE = 256
_ALIVE = []          # every allocation of the running test: a temporary handed to a launch as a bare pointer must not be recycled for the next one


class Guard:
    """checker of one guarded allocation: __call__ asserts that every element outside the interior still holds the sentinel bits"""

    def __init__(self, ints, pattern, lead, shape3, ld, bs, name):
        self.ints, self.pattern, self.lead, self.shape3, self.ld, self.bs, self.name = ints, pattern, lead, shape3, ld, bs, name
        B, L, N = shape3
        self.span = ((B - 1) * bs + L - 1) * ld + N
        rel = torch.arange(self.span, device=ints.device)
        row, col = rel // ld, rel % ld
        inside = (col < N) & (row % bs < L)
        self.outside = torch.ones(ints.numel(), dtype=torch.bool, device=ints.device)
        self.outside[lead:lead + self.span] = ~inside

    def bad(self):
        """None, or (region, row, column) of the first element outside the interior that lost the pattern; row / column count from the interior's
        first element in units of ld (negative rows: the leading guard)"""
        wrong = (self.ints != self.pattern) & self.outside
        if not bool(wrong.any()):
            return None
        off = int(torch.nonzero(wrong)[0])
        rel = off - self.lead
        row, col = rel // self.ld, rel % self.ld
        if rel < 0:
            region = "lead"
        elif rel >= self.span:
            region = "tail"
        elif col >= self.shape3[2]:
            region = "row gap"
        else:
            region = "batch gap"
        return region, row, col

    def __call__(self):
        b = self.bad()
        assert b is None, "%s: write outside the extent: region %s, row %d, column %d" % ((self.name,) + b)


def guarded(shape, dtype, ld=None, batch_stride=None, lead=LEAD, tail=None, device=dev, name="buffer"):
    """One flat allocation filled with the dtype's sentinel bit pattern -> (interior view of `shape`, Guard).
    shape (n,), (rows, N) or (B, L, N); rows are ld >= N elements apart, batches batch_stride >= L rows apart.  tail: elements behind the interior
    (default and minimum for 2-D / 3-D: 256 rows x ld - the tallest tile of any kernel; for a 1-D workspace the caller passes one more unit of its
    layout); lead and tail are never below 4096 elements."""
    shape = tuple(shape)
    shape3 = (1,) * (3 - len(shape)) + shape
    B, L, N = shape3
    ld = N if ld is None else ld
    bs = L if batch_stride is None else batch_stride
    assert ld >= N and bs >= L and lead >= LEAD
    floor = LEAD if len(shape) == 1 else max(LEAD, TALLEST_TILE * ld)
    tail = floor if tail is None else max(tail, floor)
    span = ((B - 1) * bs + L - 1) * ld + N
    it = _INT_OF[dtype]
    ints = torch.full((lead + span + tail,), SENTINEL[dtype], dtype=it, device=device)
    _ALIVE.append(ints)
    flat = ints.view(dtype)
    strides = (bs * ld, ld, 1)[3 - len(shape):]
    view = torch.as_strided(flat, shape, strides, lead)
    return view, Guard(ints, SENTINEL[dtype], lead, shape3, ld, bs, name)


def filled(t, **kw):
    """a guarded copy of host tensor t on the device (inputs: everything around the values is NaN / the integer sentinel) -> view"""
    v, _ = guarded(t.shape, t.dtype, **kw)
    v.copy_(t)
    return v
