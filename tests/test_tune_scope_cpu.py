"""_lib.set_tune / _lib.tuned on the built library, without a GPU (x2_tune is host-side state): a refused knob raises, the value that
was there before comes back - after the body, after an exception, after a refusal half way through - and a knob that already holds its
value costs no call (graph.SegmentedStep relies on that for key 12)."""
import importlib

import pytest

L = importlib.import_module("x2-vlm_amd._lib")


@pytest.fixture
def h():
    """the library handle with key 13 at 2 (not its default) for the test, every knob at its earlier value afterwards"""
    h = L.lib()
    before = {k: h.x2_tune_get(k) for k in (0, 1, 3, 5, 10, 12, 13, 14, 15)}
    assert h.x2_tune(13, 2) == 0
    yield h
    for k, v in before.items():
        assert h.x2_tune(k, v) == 0


def test_set_tune_raises_with_key_value_and_the_library_message(h):
    L.set_tune(13, 4)
    assert h.x2_tune_get(13) == 4
    with pytest.raises(L.X2HipError, match=r"x2_tune\(6, 1\): x2_tune: no key 6"):
        L.set_tune(6, 1)


def test_previous_value_is_restored_not_zero(h):
    with L.tuned({13: 4}):
        assert h.x2_tune_get(13) == 4
    assert h.x2_tune_get(13) == 2


def test_previous_value_is_restored_when_the_body_raises(h):
    with pytest.raises(ZeroDivisionError):
        with L.tuned({13: 4, 14: 1}):
            assert (h.x2_tune_get(13), h.x2_tune_get(14)) == (4, 1)
            1 / 0
    assert (h.x2_tune_get(13), h.x2_tune_get(14)) == (2, 0)


def test_nesting(h):
    with L.tuned({13: 4}):
        with L.tuned({13: 1, 5: 2}):
            assert (h.x2_tune_get(13), h.x2_tune_get(5)) == (1, 2)
        assert (h.x2_tune_get(13), h.x2_tune_get(5)) == (4, 0)
    assert (h.x2_tune_get(13), h.x2_tune_get(5)) == (2, 0)


def test_refusal_of_a_later_key_puts_the_earlier_ones_back(h):
    entered = False
    with pytest.raises(L.X2HipError, match=r"x2_tune_get\(6\)|x2_tune\(6, 1\)"):
        with L.tuned({13: 4, 6: 1}):
            entered = True
    assert not entered and h.x2_tune_get(13) == 2


@pytest.mark.parametrize("knobs,message", [({2: 4}, "X2_PROBE builds only"), ({12: -1}, "reserved compute units = -1"), ({99: 1}, "99")],
                         ids=["probe_only_key", "negative_reserve", "unknown_key"])
def test_refused_knobs_raise(h, knobs, message):
    with pytest.raises(L.X2HipError, match=message):
        with L.tuned(knobs):
            pytest.fail("the body ran under a refused knob")
    assert (h.x2_tune_get(2), h.x2_tune_get(12)) == (0, 0)


@pytest.fixture
def set_calls(h, monkeypatch):
    """x2_tune on the handle replaced by a stub that records (key, value) and passes the call on"""
    calls, real = [], h.x2_tune
    monkeypatch.setattr(h, "x2_tune", lambda k, v: calls.append((k, v)) or real(k, v))
    return calls


def test_no_set_call_when_the_value_is_already_there(h, set_calls):
    with L.tuned({13: 2}):
        assert h.x2_tune_get(13) == 2
    assert set_calls == []


def test_one_set_on_entry_and_one_on_exit_otherwise(h, set_calls):
    """graph.SegmentedStep's reserved compute units: previous value != requested"""
    with L.tuned({12: 16}):
        assert set_calls == [(12, 16)] and h.x2_tune_get(12) == 16
    assert set_calls == [(12, 16), (12, 0)] and h.x2_tune_get(12) == 0


def test_environment_knobs_go_through_the_same_check(h, monkeypatch):
    """X2_TUNE is applied when lib() first loads the library: "6=1" makes it raise (and leaves nothing loaded), a kept key is set"""
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setenv("X2_TUNE", "13=4,6=1")
    with pytest.raises(L.X2HipError, match=r"x2_tune\(6, 1\)"):
        L.lib()
    assert L._lib is None
    monkeypatch.setenv("X2_TUNE", "13=1")
    assert L.lib().x2_tune_get(13) == 1
