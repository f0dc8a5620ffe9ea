"""The guard helper of tests/test_kernel_extents_gpu.py (tests/kernel_helpers.py) on CPU tensors: an untouched buffer passes; a one-element write immediately before or after
the interior, in a row gap, in a batch gap or at the last element of the trailing guard fails and is named (region, row, column) - for every dtype,
also when the written value is itself a NaN with another payload (the comparison is on the bits)."""
import pytest
import torch

from kernel_helpers import BF16, F32, I32, I64, LEAD, SENTINEL, TALLEST_TILE, _INT_OF, guarded

B, L, N, LD, BS = 3, 5, 8, 12, 7      # rows of 8 inside 12, batches of 5 rows inside 7


def other_bits(dtype):
    """values to write, as bit patterns: an ordinary one, zero, and for the float types a NaN whose payload differs from the sentinel's in one bit"""
    vals = [1, 0]
    if dtype in (F32, BF16):
        vals.append(SENTINEL[dtype] ^ 1)
    else:
        vals.append(SENTINEL[dtype] + 1)
    return vals


@pytest.mark.parametrize("dtype", [F32, BF16, I32, I64], ids=["fp32", "bf16", "int32", "int64"])
def test_guard_catches_single_writes(dtype):
    view, chk = guarded((B, L, N), dtype, ld=LD, batch_stride=BS, device="cpu", name="t")
    assert view.shape == (B, L, N) and view.stride() == (BS * LD, LD, 1) and view.dtype == dtype
    span = ((B - 1) * BS + L - 1) * LD + N
    total = chk.ints.numel()
    assert total - LEAD - span >= TALLEST_TILE * LD and total - LEAD - span >= 4096
    if dtype in (F32, BF16):
        assert bool(torch.isnan(chk.ints.view(dtype)).all())          # the pattern is a NaN: an input read outside its extent poisons the result
    else:
        assert int(chk.ints[0]) < 0
    chk()
    view.fill_(3)                                                      # the interior is the kernel's to write
    view[1, 2, 3] = 0
    chk()
    assert chk.bad() is None
    spots = {"before": (LEAD - 1, ("lead", -1, LD - 1)),
             "after": (LEAD + span, ("tail", ((B - 1) * BS + L - 1), N)),
             "row gap": (LEAD + 2 * LD + N, ("row gap", 2, N)),
             "batch gap": (LEAD + (BS + L) * LD + 1, ("batch gap", BS + L, 1)),
             "last of the tail": (total - 1, ("tail", (total - 1 - LEAD) // LD, (total - 1 - LEAD) % LD))}
    for where, (off, want) in spots.items():
        for bits in other_bits(dtype):
            keep = int(chk.ints[off])
            chk.ints[off] = bits
            assert chk.bad() == want, (where, bits, chk.bad())
            with pytest.raises(AssertionError, match="t: write outside the extent: region %s, row %d, column %d" % want):
                chk()
            chk.ints[off] = keep
            chk()
    # the first offender is the one reported
    chk.ints[total - 1] = 1
    chk.ints[LEAD - 1] = 1
    assert chk.bad()[0] == "lead"


def test_guard_shapes_and_sizes():
    v, chk = guarded((10,), F32, tail=30, device="cpu")
    assert v.shape == (10,) and chk.ints.numel() == LEAD + 10 + 4096      # a workspace tail is never below 4096 elements
    v, chk = guarded((10,), F32, tail=65536, device="cpu")
    assert chk.ints.numel() == LEAD + 10 + 65536
    chk.ints[LEAD + 10] = 0
    assert chk.bad() == ("tail", 1, 0)
    v, chk = guarded((4, 8), BF16, ld=16, device="cpu")
    assert v.stride() == (16, 1) and chk.ints.numel() == LEAD + 3 * 16 + 8 + 256 * 16 and chk.ints.dtype == _INT_OF[BF16]
    v[3, 7] = 1.0
    chk()
    chk.ints[LEAD + 3 * 16 + 8] = 0
    assert chk.bad() == ("tail", 3, 8)
    with pytest.raises(AssertionError):
        guarded((4, 8), F32, ld=4, device="cpu")
    with pytest.raises(AssertionError):
        guarded((4,), F32, lead=16, device="cpu")
