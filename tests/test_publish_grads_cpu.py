"""The publishing rule of accelerator._Wrapped (what RocmDDPAccelerator.set_up returns): a fused model call has computed the gradients g of the
PLAIN SUM of its losses before it returns; the caller's backward through the returned loss values decides what reaches .grad.  Driven on the CPU
with a one-parameter stub: `_PublishGrads.apply(anchor, wrapped, pending, values)` is exactly what `_Wrapped.forward` ends with.

Pretrain.run_mixed_iter backpropagates iter_perc * (sum of a part's losses) for every part (Pretrain.py:197, 206, 217-223): all cotangents of a part
are then EQUAL, but not 1 - the published gradient must be iter_perc * g.  Expected gradients are formed in float64 from the held gradient and the
literal weights; the scalings used (0.5, 2, 0, and sums of two fp32 tensors) are exact or one rounding in fp32, so the comparison is to 1e-6."""
import importlib
import types

import pytest
import torch


@pytest.fixture(scope="module")
def acc():
    return importlib.import_module("x2-vlm_amd.accelerator")


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.linspace(-1.0, 1.0, 7))

    def forward(self, image, text_ids, text_atts, **kw):       # the text-only call of the wrapper's eager path
        return {"loss_mlm": (A[2] * self.w).sum()}


A = torch.tensor([[0.5, -1.0, 2.0, 0.25, 3.0, -0.75, 1.5],        # loss_i = (A[i] * w).sum(): d loss_i / d w = A[i]
                  [1.0, 4.0, -2.0, 0.5, -0.125, 2.5, -3.0],
                  [-1.5, 0.75, 1.0, -4.0, 2.0, 0.375, 0.5]])


def _fused_call(acc, wrapped, g, call=None, step=None):
    """The tail of _Wrapped.forward: loss values tied to a pending set of already-computed gradients."""
    p = wrapped.module.w
    anchor = torch.zeros((), requires_grad=True)
    values = torch.tensor([1.0, 2.0, 3.0])
    pending = dict(held=[(p, g)], call=call, step=step)
    return acc._PublishGrads.apply(anchor, wrapped, pending, values), pending


def _counting_call(module):
    n = [0]

    def call():
        n[0] += 1
        return {"loss_%d" % i: (A[i] * module.w).sum() for i in range(3)}
    return call, n


def _close(got, want64):
    return got is not None and float((got.double() - want64).abs().max()) <= 1e-6 * max(1.0, float(want64.abs().max()))


def test_plain_sum_publishes_the_held_tensor_itself(acc):
    wrapped = acc._Wrapped(_Stub(), None)
    g = A.sum(0).clone()
    want = g.double().clone()
    step = types.SimpleNamespace(_busy=True)
    (o0, o1, o2), pending = _fused_call(acc, wrapped, g, step=step)
    assert wrapped.has_pending()
    assert wrapped.module.w.grad is None                       # out of reach until the backward
    (o0 + o1 + o2).backward()
    assert wrapped.module.w.grad is g                          # the optimizer reads a step's static gradient tensors by identity
    assert _close(g, want)
    assert step._busy is False and pending["held"] is None and not wrapped.has_pending()


@pytest.mark.parametrize("c", [0.5, 2.0, 0.0])
def test_uniform_weight_scales_the_published_gradient(acc, c):
    """c * (l0 + l1 + l2): every cotangent is c.  (c = 0.5 is the region part of configs/pretrain/x2vlm_base_1b.yaml.)"""
    wrapped = acc._Wrapped(_Stub(), None)
    g = A.sum(0).clone()
    want = c * A.sum(0).double()
    call, n = _counting_call(wrapped.module)
    (o0, o1, o2), _ = _fused_call(acc, wrapped, g, call=call)
    (c * (o0 + o1 + o2)).backward()
    got = wrapped.module.w.grad
    assert _close(got, want), (c, got, want)
    assert got is g                                            # scaled in place: still the held tensor
    assert n[0] == 0                                           # nothing was recomputed


def test_unequal_weights_recompute_with_the_callers_weights(acc):
    wrapped = acc._Wrapped(_Stub(), None)
    w = (1.0, 0.5, 2.0)
    want = sum(wi * A[i].double() for i, wi in enumerate(w))
    call, n = _counting_call(wrapped.module)
    (o0, o1, o2), _ = _fused_call(acc, wrapped, torch.full((7,), 1e3), call=call)      # the held gradient must NOT be used
    (w[0] * o0 + w[1] * o1 + w[2] * o2).backward()
    assert n[0] == 1
    assert _close(wrapped.module.w.grad, want)
    assert wrapped._local                                      # this rank's own gradients: backward_step averages them


def test_a_loss_left_out_of_the_sum_recomputes(acc):
    """regions_use_bbox_only (Pretrain.py:216-218): some of the returned losses never enter the total - their cotangent is None."""
    wrapped = acc._Wrapped(_Stub(), None)
    want = (A[0] + A[2]).double()
    call, n = _counting_call(wrapped.module)
    (o0, o1, o2), _ = _fused_call(acc, wrapped, torch.full((7,), 1e3), call=call)
    (o0 + o2).backward()
    assert n[0] == 1
    assert _close(wrapped.module.w.grad, want)


def test_two_pending_calls_published_by_one_backward(acc):
    """The image part (weight 1) and the region part (weight 0.5) of run_mixed_iter: two fused calls, one backward_step."""
    wrapped = acc._Wrapped(_Stub(), None)
    g1, g2 = A[0].clone(), A[1].clone()
    want = A[0].double() + 0.5 * A[1].double()
    a, _ = _fused_call(acc, wrapped, g1)
    b, _ = _fused_call(acc, wrapped, g2)
    assert wrapped.has_pending()
    (1.0 * (a[0] + a[1] + a[2]) + 0.5 * (b[0] + b[1] + b[2])).backward()
    assert _close(wrapped.module.w.grad, want)
    assert not wrapped.has_pending()


def test_two_backward_calls_without_zero_grad_accumulate(acc):
    """The video part has a backward_step of its own (Pretrain.py:197) before the main one (:247), one zero_grad before both."""
    wrapped = acc._Wrapped(_Stub(), None)
    g1, g2 = A[0].clone(), A[1].clone()
    want = A[0].double() + 0.5 * A[1].double()
    b, _ = _fused_call(acc, wrapped, g2)
    (0.5 * (b[0] + b[1] + b[2])).backward()
    assert _close(wrapped.module.w.grad, 0.5 * A[1].double())
    a, _ = _fused_call(acc, wrapped, g1)
    (1.0 * (a[0] + a[1] + a[2])).backward()
    assert _close(wrapped.module.w.grad, want)


def test_second_backward_through_the_same_losses_raises(acc):
    wrapped = acc._Wrapped(_Stub(), None)
    (o0, o1, o2), _ = _fused_call(acc, wrapped, A[0].clone())
    total = o0 + o1 + o2
    total.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match="second backward"):
        total.backward()


class _CountingBuckets:
    def __init__(self):
        self.finished = 0

    def finish(self):
        self.finished += 1


def test_backward_step_averages_whenever_this_ranks_own_gradients_were_produced(acc):
    """More than one rank: fused calls come back averaged and backward_step has nothing to reduce - unless the same iteration also produced this
    rank's own gradients: a recomputed backward (unequal / None cotangents), or an eager call anywhere in it (the text part of run_mixed_iter,
    which sets last_mode to "eager" only when it happens to be the last call)."""
    a = acc.RocmDDPAccelerator(dict(), None)
    wrapped = a.ddp_model = acc._Wrapped(_Stub(), a)
    a.buckets = _CountingBuckets()
    call, _ = _counting_call(wrapped.module)
    # fused calls only, uniform weight: published, nothing to reduce
    (o0, o1, o2), _ = _fused_call(acc, wrapped, A[0].clone(), call=call)
    wrapped.last_mode = "hipgraph-segments"
    a.backward_step(0.5 * (o0 + o1 + o2))
    assert a.buckets.finished == 0
    # a loss left out: recomputed eagerly inside the backward -> reduced
    (o0, o1, o2), _ = _fused_call(acc, wrapped, A[0].clone(), call=call)
    a.backward_step(o0 + o2)
    assert a.buckets.finished == 1 and not wrapped._local
    # an eager call with gradients FOLLOWED by a fused call: last_mode alone would skip the reduction
    loss = wrapped(None, text_ids=None)
    assert wrapped.last_mode == "eager" and wrapped._local
    (o0, o1, o2), _ = _fused_call(acc, wrapped, A[0].clone(), call=call)
    wrapped.last_mode = "hipgraph-segments"
    a.backward_step(loss["loss_mlm"] + (o0 + o1 + o2))
    assert a.buckets.finished == 2 and not wrapped._local
    # and the next all-fused backward is left alone again
    (o0, o1, o2), _ = _fused_call(acc, wrapped, A[0].clone(), call=call)
    a.backward_step(o0 + o1 + o2)
    assert a.buckets.finished == 2
