"""radnerf/step_graphs.py without a GPU: the held device scalar, the static inputs' feed() rules and the bounded least-recently-used
cache of captured steps, driven with CPU tensors and stand-in graphs; and a Trainer assembled without __init__, as bench.py's eager
probe assembles one, taking a step.  What GraphedTrainer captures and replays through them is held to the eager trainer on the GPU
(tests/test_gpu_lips_graph.py, tests/test_gpu_train.py)."""
import contextlib
import os
import sys
from unittest import mock

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "rad-nerf_amd"))

from radnerf.step_graphs import GraphCache, HeldScalar, StaticInputs  # noqa: E402

# the keys of tests/test_gpu_lips_graph.py's rect schedule at one row capacity: A2 is A's shape elsewhere, so it has A's key
RAYS, RAYS_S = (1, 1280, 3), (1, 961, 3)
PLAIN = (16384, (1, 1024, 3))
A, T, S = (16384, RAYS, "rect", (32, 40)), (16384, RAYS, "rect", (40, 32)), (16384, RAYS_S, "rect", (31, 31))
SCHEDULE = [PLAIN, A, PLAIN, T, PLAIN, A, PLAIN, S, PLAIN, A, PLAIN, T]


def _layout(key):
    return ("plain", key[1]) if len(key) == 2 else key[-3:]


class _Recorder:
    """Stands in for GraphedTrainer._capture: a new object per graph, new static inputs where the cache holds none."""

    def __init__(self):
        self.calls = []

    def capture(self, key):
        def run(held):
            self.calls.append((key, held))
            return object(), object(), held if held is not None else object()
        return run


@pytest.mark.parametrize("bound, captured", [(4, [A, T, S]), (2, [A, T, S, T]), (1, [A, T, A, S, A, T])])
def test_the_rect_schedule_in_least_recently_used_order(bound, captured):
    """With 4 slots A, T and S are captured once each; with 2 the order evicts T for S, then S for T.  The key just asked for is
    the newest entry and is never the one evicted."""
    plain, lips, rec = GraphCache(8), GraphCache(bound), _Recorder()
    held_after = []
    for key in SCHEDULE:
        cache = plain if key is PLAIN else lips
        graph, loss, inputs = cache.get(key, _layout(key), rec.capture(key))
        assert list(cache.graphs)[-1] == key and cache.newest() == (graph, loss, inputs)
        assert len(lips.graphs) <= bound and set(lips.inputs) == {e[2] for e in lips.graphs.values()}
        held_after.append(list(lips.graphs))
    assert [k for k, _ in rec.calls if k is not PLAIN] == captured
    assert [k for k, _ in rec.calls if k is PLAIN] == [PLAIN] and list(plain.graphs) == [PLAIN]
    if bound == 2:
        assert held_after[7] == [A, S] and held_after[9] == [S, A] and held_after[11] == [A, T]


def test_a_hit_returns_what_the_capture_returned():
    cache, rec = GraphCache(2), _Recorder()
    first = cache.get(A, _layout(A), rec.capture(A))
    cache.get(T, _layout(T), rec.capture(T))
    assert cache.get(A, _layout(A), rec.capture(A)) == first and len(rec.calls) == 2
    assert list(cache.graphs) == [T, A]


def test_a_bound_of_zero_still_keeps_the_newest():
    cache, rec = GraphCache(0), _Recorder()
    for key in (A, S, A):
        cache.get(key, _layout(key), rec.capture(key))
        assert list(cache.graphs) == [key] and list(cache.inputs) == [_layout(key)]
    assert len(rec.calls) == 3


def test_keys_of_one_layout_share_their_static_inputs():
    """Two row capacities of layout L read one set; it goes exactly when the second of them is evicted."""
    L, M = (RAYS, "rect", (32, 40)), (RAYS_S, "rect", (31, 31))
    k1, k2, k3, k4 = (16384,) + L, (20480,) + L, (16384,) + M, (20480,) + M
    cache, rec = GraphCache(2), _Recorder()
    _, _, first = cache.get(k1, L, rec.capture(k1))
    assert rec.calls[-1] == (k1, None)
    _, _, second = cache.get(k2, L, rec.capture(k2))
    assert rec.calls[-1] == (k2, first) and second is first and list(cache.inputs) == [L]
    cache.get(k3, M, rec.capture(k3))                           # evicts k1: k2 still reads L's inputs
    assert list(cache.graphs) == [k2, k3] and cache.inputs[L] is first and set(cache.inputs) == {L, M}
    cache.get(k2, L, rec.capture(k2))                           # a hit: nothing is captured, nothing released
    assert len(rec.calls) == 3 and set(cache.inputs) == {L, M}
    cache.get(k4, M, rec.capture(k4))                           # evicts k3: M stays (k4 reads it)
    assert list(cache.graphs) == [k2, k4] and set(cache.inputs) == {L, M} and rec.calls[-1][1] is not None
    cache.get(k3, M, rec.capture(k3))                           # evicts k2, the last graph of L
    assert list(cache.graphs) == [k4, k3] and set(cache.inputs) == {M}
    _, _, again = cache.get(k1, L, rec.capture(k1))             # L comes back with inputs of its own
    assert rec.calls[-1] == (k1, None) and again is not first


def test_held_scalar_fills_only_when_the_value_moved():
    h = HeldScalar(1, torch.int32, "cpu")
    assert h.value is None and h.tensor.shape == (1,) and h.tensor.dtype == torch.int32
    assert h.set(0) is h.tensor and h.value == 0                # the first value is always written, a zero too
    assert h.set(12032) is h.tensor and int(h.tensor) == 12032
    h.tensor.zero_()
    h.set(12032)
    assert int(h.tensor) == 0                                   # the same value: no fill
    h.set(12160)
    assert int(h.tensor) == 12160 and h.value == 12160
    w = HeldScalar((), torch.float32, "cpu")
    assert w.tensor.shape == () and float(w.set(0.025)) == pytest.approx(0.025)


@contextlib.contextmanager
def _copies():
    """-> the list of (destination, source) of every Tensor.copy_ inside the block."""
    calls, real = [], torch.Tensor.copy_

    def spy(self, src, *a, **kw):
        calls.append((self, src))
        return real(self, src, *a, **kw)
    with mock.patch.object(torch.Tensor, "copy_", spy):
        yield calls


class _Frames:
    """Packed batches as SyntheticTrainStream / DeviceTrainSet hand them out: per-ray sections as views of one flat buffer, the
    per-frame tensors of a frame the same objects in every batch of that frame."""

    def __init__(self, n):
        self.n = n
        self.per_frame = {f: dict(poses=torch.full((1, 6), float(f)), eye=torch.full((1, 1), float(f)), auds=torch.full((1, 4), float(f)))
                          for f in range(3)}

    def unpack(self, flat, frame=0):
        n = self.n
        return dict(rays_o=flat[:3 * n].view(1, n, 3), images=flat[3 * n:].view(1, n, 3), index=[frame], _packed=flat,
                    _unpack=self.unpack, **self.per_frame[frame])

    def batch(self, frame, seed, index_dev=False):
        flat = torch.rand(6 * self.n, generator=torch.Generator().manual_seed(seed))
        b = self.unpack(flat, frame)
        if index_dev:
            b["_index_dev"] = torch.tensor([frame], dtype=torch.long)
        return b


def test_feed_of_a_packed_batch():
    frames = _Frames(5)
    first = frames.batch(0, 1)
    inputs = StaticInputs(first, "cpu")
    st = inputs.static
    assert st["_packed"] is not first["_packed"] and torch.equal(st["_packed"], first["_packed"]) and inputs.budget is None
    assert st["rays_o"].data_ptr() == st["_packed"].data_ptr()                   # the step's inputs are views of the one clone
    assert inputs.index == [0] and st["index"].dtype == torch.long and st["index"].tolist() == [0]
    assert st["poses"] is first["poses"]
    # the same frame again: the packed rows and nothing else
    second = frames.batch(0, 2)
    with _copies() as calls:
        inputs.feed(second)
    assert [(d is st["_packed"], s is second["_packed"]) for d, s in calls] == [(True, True)]
    assert torch.equal(st["rays_o"], second["rays_o"]) and torch.equal(st["images"], second["images"]) and inputs.index == [0]
    # another frame: its per-frame tensors are other tensors and are copied, the index comes from the list
    third = frames.batch(2, 3)
    with _copies() as calls:
        inputs.feed(third)
    assert [d is st[k] and s is third[k] for (d, s), k in zip(calls, ("_packed", "poses", "eye", "auds"))] == [True] * 4
    assert len(calls) == 5 and calls[4][0] is st["index"] and st["index"].tolist() == [2] and inputs.index == [2]
    assert float(st["poses"][0, 0]) == 2.0
    # ... or from the batch's device tensor where it brings one
    fourth = frames.batch(1, 4, index_dev=True)
    with _copies() as calls:
        inputs.feed(fourth)
    assert calls[-1][0] is st["index"] and calls[-1][1] is fourth["_index_dev"] and inputs.index == [1] and st["index"].tolist() == [1]
    # an unchanged index list copies nothing into the index, whatever the tensor holds
    st["index"].fill_(77)
    with _copies() as calls:
        inputs.feed(frames.batch(1, 5, index_dev=True))
    assert all(d is not st["index"] for d, _ in calls) and st["index"].tolist() == [77]


def test_feed_of_a_batch_of_separate_tensors():
    g = torch.Generator().manual_seed(0)
    make = lambda frame: dict(rays_o=torch.rand(1, 7, 3, generator=g), face_mask=torch.rand(1, 7, generator=g) > 0.5,
                              poses=torch.rand(1, 6, generator=g), index=[frame], rect=(1, 2, 3, 10), bg_color=None)
    first = make(4)
    budget = (torch.tensor([128], dtype=torch.int32), 128, True)
    inputs = StaticInputs(first, "cpu", budget)
    st = inputs.static
    assert inputs.budget is budget and st["rect"] == (1, 2, 3, 10) and st["bg_color"] is None
    assert all(st[k] is not first[k] and torch.equal(st[k], first[k]) for k in ("rays_o", "face_mask", "poses"))
    second = make(6)
    with _copies() as calls:
        inputs.feed(second)
    assert [(d is st[k], s is second[k]) for (d, s), k in zip(calls, ("rays_o", "face_mask", "poses"))] == [(True, True)] * 3
    assert len(calls) == 4 and calls[3][0] is st["index"] and st["index"].tolist() == [6] and inputs.index == [6]
    assert all(torch.equal(st[k], second[k]) for k in ("rays_o", "face_mask", "poses"))
    # a batch whose index is a tensor already: copied as every tensor entry is, no list is held
    tensor_index = dict(first, index=torch.tensor([3]))
    inputs = StaticInputs(tensor_index, "cpu")
    assert inputs.index is None
    inputs.feed(dict(second, index=torch.tensor([5])))
    assert inputs.static["index"].tolist() == [5] and inputs.index is None


def test_a_trainer_assembled_without_init_takes_a_step():
    """bench.py's eager probe: Trainer.__new__ around another trainer's model and optimizer.  The class defaults stand in for what
    __init__ would have set, the device budget among them (made at the first step that has one: none on a CPU model)."""
    import radnerf.train as train
    from test_lips_graph_host import OPT, _step_inputs, _Stub
    out, data = _step_inputs(48, 3)
    m = _Stub(out)
    first = train.Trainer(m, OPT, prefer_rocblas=False, update_extra_interval=0)
    first.step(data)
    t = train.Trainer.__new__(train.Trainer)
    t.model, t.opt, t.optimizer, t.update_extra_interval = m, OPT, first.optimizer, 0
    t.iters, t.lambda_amb, t.global_step = first.iters, first.lambda_amb, first.global_step
    assert t._budget is None and t.patch_criterion is None and t.ema is None and t.lr_gamma is None and not t._device_schedule
    before = m.w.detach().clone()
    loss = t.step(data)
    assert torch.isfinite(loss) and not loss.requires_grad and t.global_step == 2 and not torch.equal(m.w.detach(), before)
    assert t._device_budget(m) is None and t._budget is None
    m.mean_count = 12000                                         # a budget, but no device to hold it
    assert t._device_budget(m) is None
    with t.eval_scope():
        assert not m.training and not torch.is_grad_enabled()
    assert m.training
    assert train.make_optimizer.__module__ == "radnerf.optim" and train.HipAdam.__module__ == "radnerf.optim"
