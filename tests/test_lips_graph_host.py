"""GraphedTrainer's opt-in captured lip fine-tuning steps (lips_graphs) and DeviceTrainSet.lips_shapes() without a GPU: the
argument, the class default, the eager step a CPU model keeps for such batches, and the count of rect shapes.  What is captured
and replayed is held to the eager trainer on the GPU (tests/test_gpu_lips_graph.py)."""
import collections
import types

import pytest
import torch

import lips_cases as lc


@pytest.fixture(scope="module")
def _pkg(hiplib):
    import radnerf.train as train
    return train


class _Stub(torch.nn.Module):
    """A stand-in model of the kind tests/test_train_set_lips_host.py uses: render() hands back fixed outputs scaled by one
    parameter; no sample budget yet (mean_count = 0), as a model in its first window."""
    mean_count = 0

    def __init__(self, out):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))
        self.out, self.kwargs = out, None

    def render(self, *a, **kw):
        self.kwargs = kw
        return {k: v * self.w for k, v in self.out.items()}

    def get_params(self, lr, lr_net, wd=0):
        return [{"params": [self.w], "lr": lr_net}]


def _criterion(pred, target):
    return (pred - target).abs().mean(dim=(1, 2, 3), keepdim=True)


def _step_inputs(N, seed):
    g = torch.Generator().manual_seed(seed)
    out = dict(image=torch.rand(1, N, 3, generator=g), weights_sum=torch.rand(N, generator=g), ambient=torch.rand(N, generator=g))
    data = dict(rays_o=None, rays_d=None, auds=None, bg_coords=None, poses=None, eye=None, index=[0], bg_color=None,
                images=torch.rand(1, N, 3, generator=g), face_mask=torch.rand(1, N, generator=g) > 0.5)
    return out, data


OPT = types.SimpleNamespace(torso=False, dt_gamma=1 / 256, max_steps=16)


def test_a_negative_lips_graphs_is_an_error(_pkg):
    out, _ = _step_inputs(35, 3)
    with pytest.raises(ValueError, match="lips_graphs"):
        _pkg.GraphedTrainer(_Stub(out), OPT, prefer_rocblas=False, lips_graphs=-1)


def test_the_class_default_is_no_lips_graphs(_pkg):
    """bench.py assembles trainers without __init__: such a trainer refuses a lips batch as it always did."""
    out, data = _step_inputs(35, 3)
    assert _pkg.GraphedTrainer.lips_graphs == 0 and _pkg.GraphedTrainer.__new__(_pkg.GraphedTrainer).lips_graphs == 0
    t = _pkg.GraphedTrainer(_Stub(out), OPT, prefer_rocblas=False)
    assert t.lips_graphs == 0 and t.lips_captures == 0 and t.lips_capture_log == []
    with pytest.raises(ValueError, match="lip fine-tuning batch"):
        t.step(dict(data, rect=(3, 8, 2, 9)))


@pytest.mark.parametrize("criterion", [None, _criterion])
def test_a_cpu_model_takes_lips_batches_through_the_eager_step(_pkg, criterion):
    """With lips_graphs > 0 nothing is refused; the first window and a CPU model keep the eager step, for a rect and for a patch
    batch, and a patch batch still marches all rays there."""
    out, data = _step_inputs(48, 3)
    m = _Stub(out)
    t = _pkg.GraphedTrainer(m, OPT, prefer_rocblas=False, update_extra_interval=0, patch_criterion=criterion, lips_graphs=2)
    assert t.lips_graphs == 2
    for step, (extra, forced) in enumerate([(dict(rect=(3, 9, 2, 10)), False), (dict(patch_size=4), True), ({}, False)]):
        before = m.w.detach().clone()
        loss = t.step(dict(data, **extra))
        assert torch.isfinite(loss) and t.global_step == step + 1 and m.kwargs["force_all_rays"] is forced
        assert not torch.equal(m.w.detach(), before)
    assert t.captures == t.replays == t.lips_captures == 0 and t.capture_log == [] and t.lips_capture_log == []


def test_lips_shapes_counts_the_rects(_pkg):
    ds = lc.make_set("cpu", False, 2)
    want = collections.Counter((r[1] - r[0], r[3] - r[2]) for r in ds.lips_rect)
    got = ds.lips_shapes()
    assert got == dict(want) and sum(got.values()) == ds.F and len(got) >= 2
    for f in range(ds.F):                                        # the shapes are those batch_rect() hands out
        xmin, xmax, ymin, ymax = ds.batch_rect([f])["rect"]
        assert (xmax - xmin, ymax - ymin) in got
    with pytest.raises(ValueError, match="no lips_rect"):
        lc.make_set("cpu", False, 2, lips=False).lips_shapes()
