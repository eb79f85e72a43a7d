"""radnerf/frame_cache.py without a GPU: the build-on-second-sight rule of a Slot under both capture policies, the wait-once
ordering of a second stream behind a build, the lifetime of the tensors a key names, the per-model owner under copy.deepcopy and
the lazily read LoopStats, driven with stand-in streams, events, tensors and builders.  What the fused engine builds through them
is held to its off switches on the GPU (tests/test_gpu_torso_plan.py, tests/test_gpu_dense_levels.py)."""
import copy
import gc
import os
import sys
import weakref

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))

from radnerf.frame_cache import Built, FrameCaches, LoopStats, Slot  # noqa: E402


class _Tensor:
    """Stands in for a tensor: weakly referencable, remembers the streams it was recorded on."""

    def __init__(self):
        self.recorded = []

    def record_stream(self, stream):
        self.recorded.append(stream)


class _Stream:
    def __init__(self, handle):
        self.cuda_stream, self.waits = handle, []

    def wait_event(self, event):
        self.waits.append(event)


class _Builder:
    """Stands in for FusedState._build_plan / _build_dense: a record made through the slot, on stream 1, with `n` buffers
    (0: the build yielded nothing)."""

    def __init__(self, slot, n=1):
        self.slot, self.n, self.calls = slot, n, []

    def build(self, key, refs):
        def run():
            self.calls.append(key)
            return self.slot.record(key, refs, [_Tensor() for _ in range(self.n)], object(), 1, n_on=7)
        return run

    def get(self, key, refs=(), capturing=False):
        return self.slot.get(key, refs, self.build(key, refs), capturing)


@pytest.mark.parametrize("use_under_capture", [True, False])
def test_first_sight_remembers_second_sight_builds_then_the_record_is_reused(use_under_capture):
    slot = Slot(use_under_capture)
    b = _Builder(slot)
    assert b.get("A") is None and slot.held is None and slot.builds == 0 and b.calls == []
    rec = b.get("A")
    assert isinstance(rec, Built) and rec is slot.held and rec.key == "A" and rec.n_on == 7 and rec.waited == {1}
    assert slot.builds == 1 and b.calls == ["A"]
    for _ in range(3):
        assert b.get("A") is rec
    assert slot.builds == 1 and b.calls == ["A"]


def test_a_changed_key_drops_the_record_and_the_call_after_it_builds():
    slot = Slot(True)
    b = _Builder(slot)
    b.get("A")
    first = b.get("A")
    assert b.get("B") is None and slot.held is None and slot.builds == 1          # dropped; this call builds nothing
    second = b.get("B")
    assert second is not None and second is not first and second.key == "B" and slot.builds == 2 and b.calls == ["A", "B"]
    assert b.get("A") is None and b.get("B") is None and slot.builds == 2         # back and forth: dropped, then only remembered
    assert b.get("B") is not None and slot.builds == 3


def test_alternating_and_ever_changing_keys_never_build():
    slot = Slot(True)
    b = _Builder(slot)
    for i in range(8):
        assert b.get("AB"[i & 1]) is None
    for i in range(8):
        assert b.get(("moving", i)) is None
    assert slot.builds == 0 and b.calls == [] and slot.held is None


def test_an_empty_build_is_held_and_not_tried_again():
    slot = Slot(True)
    b = _Builder(slot, n=0)
    assert b.get("A") is None and b.get("A") is None                              # the second call built: nothing came of it
    assert slot.builds == 1 and slot.held is not None and slot.held.key == "A" and slot.held.tensors == ()
    for _ in range(4):
        assert b.get("A") is None
    assert slot.builds == 1 and b.calls == ["A"]
    assert b.get("B") is None and slot.held is None                               # ... and is dropped like any other
    assert b.get("B") is None and slot.builds == 2


def test_a_slot_that_may_be_used_under_capture_hands_out_but_never_builds():
    slot = Slot(use_under_capture=True)
    b = _Builder(slot)
    assert b.get("A", capturing=True) is None
    for _ in range(3):                                                            # seen on the call before, yet no build
        assert b.get("A", capturing=True) is None
    assert slot.builds == 0 and b.calls == [] and slot.seen[0] == "A"
    rec = b.get("A")                                                              # the capturing calls did remember the key
    assert rec is not None and slot.builds == 1
    assert b.get("A", capturing=True) is rec                                      # a held record is handed out
    assert b.get("B", capturing=True) is None and slot.held is None               # a changed key drops it under capture too
    assert b.get("B", capturing=True) is None and slot.builds == 1
    assert b.get("B") is not None and slot.builds == 2


def test_a_slot_that_may_not_be_used_under_capture_is_left_untouched_by_a_capturing_call():
    slot = Slot(use_under_capture=False)
    b = _Builder(slot)
    assert b.get("A", capturing=True) is None and slot.seen is None               # not even remembered
    assert b.get("A") is None and slot.builds == 0                                # so this is the first sight
    rec = b.get("A")
    assert rec is not None and slot.builds == 1
    seen = slot.seen
    assert b.get("A", capturing=True) is None and slot.held is rec                # held, but not handed out
    assert b.get("B", capturing=True) is None and slot.held is rec and slot.seen is seen      # nor dropped, nor remembered
    assert b.get("A") is rec and slot.builds == 1 and b.calls == ["A"]


def test_forget_empties_the_slot_and_keeps_the_count():
    slot = Slot(True)
    b = _Builder(slot)
    b.get("A"), b.get("A")
    slot.forget()
    assert slot.held is None and slot.seen is None and slot.builds == 1
    assert b.get("A") is None and b.get("A") is not None and slot.builds == 2


def test_a_second_stream_waits_once_and_records_every_tensor_once():
    slot = Slot(True)
    b = _Builder(slot, n=2)
    b.get("A")
    rec = b.get("A")
    builder_stream, side = _Stream(1), _Stream(2)
    rec.order(builder_stream)                                                     # the stream of the build: nothing to order
    assert builder_stream.waits == [] and all(t.recorded == [] for t in rec.tensors) and rec.waited == {1}
    rec.order(side)
    assert side.waits == [rec.event] and [t.recorded for t in rec.tensors] == [[side], [side]] and rec.waited == {1, 2}
    rec.order(side)
    rec.order(_Stream(2))                                                         # the handle counts, not the wrapper
    assert side.waits == [rec.event] and [t.recorded for t in rec.tensors] == [[side], [side]] and rec.waited == {1, 2}
    third = _Stream(3)
    rec.order(third)
    assert third.waits == [rec.event] and [t.recorded for t in rec.tensors] == [[side, third]] * 2 and rec.waited == {1, 2, 3}


def test_refs_live_while_remembered_or_held_and_go_after_a_drop():
    slot = Slot(True)
    b = _Builder(slot)
    t = _Tensor()
    alive = weakref.ref(t)
    b.get("A", [t])
    del t
    gc.collect()
    assert alive() is not None                                                    # remembered: its address cannot come back
    rec = b.get("A", [alive()])
    gc.collect()
    assert alive() is not None and rec.refs[0] is alive()                         # held
    del rec
    assert b.get("B", [_Tensor()]) is None                                        # dropped, and B is what is remembered now
    gc.collect()
    assert alive() is None
    u = _Tensor()
    gone = weakref.ref(u)
    b.get("C", [u])                                                               # remembered only ...
    del u
    b.get("D")                                                                    # ... until another key is
    gc.collect()
    assert gone() is None


class _Module:
    pass


def test_a_deep_copy_starts_with_an_empty_owner():
    m = _Module()
    m.weight, m.cache = [1.0, 2.0], FrameCaches()
    own = m.cache
    own.states[0], own.loop_hint = object(), 5
    b = _Builder(own.plan)
    b.get("A"), b.get("A")
    _Builder(own.image).get("T")
    assert own.plan.use_under_capture is True and own.image.use_under_capture is False
    c = copy.deepcopy(m)
    assert c.weight == m.weight and c.weight is not m.weight
    new = c.cache
    assert isinstance(new, FrameCaches) and new is not own and new.states == {} and new.loop_hint is None
    for slot in (new.plan, new.image):
        assert slot.held is None and slot.seen is None and slot.builds == 0
    assert new.plan.use_under_capture is True and new.image.use_under_capture is False
    assert own.plan.held is not None and own.plan.builds == 1 and own.image.seen[0] == "T" and len(own.states) == 1      # untouched


class _State:
    """Stands in for FusedState.read_loop_stats: counts its reads."""

    def __init__(self, **numbers):
        self.numbers, self.reads = numbers, 0

    def read_loop_stats(self):
        self.reads += 1
        return dict(self.numbers)


def test_loop_stats_read_once_at_the_first_access():
    numbers = dict(iterations=9, live_samples=1234, sample_slots=2048)
    st = _State(**numbers)
    stats = LoopStats(st)
    assert st.reads == 0
    assert stats["iterations"] == 9 and st.reads == 1
    assert dict(stats) == numbers and len(stats) == 3 and "live_samples" in stats and "rays" not in stats
    assert stats == numbers and stats == LoopStats(_State(**numbers)) and stats != dict(numbers, iterations=8)
    assert dict(stats) == dict(LoopStats(_State(**numbers))) and stats.get("rays", 0) == 0 and list(stats) == list(numbers)
    assert repr(stats) == repr(numbers) and st.reads == 1
    with pytest.raises(KeyError):
        stats["rays"]
    with pytest.raises(TypeError):
        hash(stats)
    for first in (len, dict, repr, list, lambda s: "iterations" in s, lambda s: s == numbers):
        st = _State(**numbers)
        stats = LoopStats(st)
        first(stats), first(stats)
        assert st.reads == 1, first
