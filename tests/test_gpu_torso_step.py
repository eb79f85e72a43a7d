"""A torso training step that stays on the device (opt-in RN_TORSO_TRAIN=fused): rn_torso_select, rn_train_torso_loss, the route
through NeRFRenderer / train_step and its capture in a graph (csrc/rn_torso.hip, csrc/rn_train_torso.hip, radnerf/train_torso.py).

Truth and bars are test_gpu_torso.py's: the coverage of rn_torso_mask + torch.nonzero bit for bit, the float64 restatement
netref64.Net64.forward_torso, and e_kernel <= 4 e_torch + 1e-6 (_compare) with today's PyTorch formulation as e_torch.

Sizes: k_torso_select is ONE workgroup of 1024 threads that walks the pixels 1024 at a time, so 1023 / 1024 / 1025 are its
workgroup edges (one round, one round exactly, a second ragged round), 63 / 64 / 65 and 255 / 256 / 257 wave edges inside a round
and 4097 four rounds and one pixel.  k_train_torso_loss is one workgroup of 1024 threads with a grid-stride loop: 1, 65, 1025, 4097."""
import contextlib

import numpy as np
import pytest
import torch

import netref64
from test_gpu_options import _maxerr
from test_gpu_torso import (PAD, THRESH, _code, _collect, _compare, _gen, _grad_names, _occupancy, _pixels, _poses, _quadrants,
                            _smooth_batch, _spy, _train_scene)

pytestmark = pytest.mark.gpu

ROW = 3
MARK, INSIDE = -77, -55


def _env(monkeypatch, fused, mlp=None):
    for name, value in (("RN_TORSO_TRAIN", "fused" if fused else None), ("RN_MLP_TRAIN", mlp)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


class _Guard:
    """alloc() of train_torso.select / torso_loss: every buffer the kernels write is cut out of a larger one, PAD rows of a marker
    on either side and another marker inside, so that rows a kernel must not write are seen to keep it."""

    def __init__(self):
        self.full = []

    def new(self, n, *tail, dtype=torch.float32):
        full = torch.full((n + 2 * PAD, *tail), MARK, dtype=dtype, device="cuda")
        view = full[PAD:PAD + n]
        view.fill_(INSIDE)
        self.full.append((full, n))
        assert view.is_contiguous()
        return view

    def check(self):
        for full, n in self.full:
            assert bool((full[:PAD] == MARK).all()) and bool((full[PAD + n:] == MARK).all()), "write outside the buffer"


def _coverages(N, gen):
    one = lambda i: torch.zeros(N, dtype=torch.bool, device="cuda").index_fill_(0, torch.tensor([i], device="cuda"), True)  # noqa: E731
    return [("half", torch.rand(N, device="cuda", generator=gen) < 0.5), ("all", torch.ones(N, dtype=torch.bool, device="cuda")),
            ("none", torch.zeros(N, dtype=torch.bool, device="cuda")), ("first", one(0)), ("last", one(N - 1))]


def _check_select(m, xy, thresh, what):
    """select() on guarded buffers against occupancy.torso_pixels (rn_torso_mask + torch.nonzero) at `thresh`; -> the index list."""
    from radnerf import occupancy, train_torso
    idx = occupancy.torso_pixels(m, xy, thresh)
    gd = _Guard()
    covered, xy_c, count = train_torso.select(m, xy, alloc=gd.new)
    gd.check()
    k = int(count[0])
    assert k == idx.numel(), (what, k, idx.numel())
    assert covered.dtype == torch.int32 and torch.equal(covered[:k].long(), idx), what
    assert torch.equal(xy_c[:k], xy[idx]), what
    assert bool((covered[k:] == INSIDE).all()) and bool((xy_c[k:] == INSIDE).all()), (what, "rows past the count were written")
    return idx


# ================================================================================================================ select
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097])
def test_select_equals_the_mask_route(hiplib, N):
    """covered[:count], xy_c[:count] and count against rn_torso_mask + torch.nonzero, bit for bit, for every coverage pattern;
    rows past the count and the margins of all three buffers untouched."""
    m = _train_scene(8).model
    gen = _gen(300 + N)
    with _occupancy(m, _quadrants()):
        assert m._mean_density_torso_dev is None                     # the host value: the kernel gets a null pointer
        for name, mask in _coverages(N, gen):
            xy = _pixels(mask, gen)
            idx = _check_select(m, xy, THRESH, (N, name))
            assert torch.equal(idx, torch.nonzero(mask).reshape(-1)), (N, name)


def test_select_takes_the_smaller_threshold_from_the_device(hiplib):
    """Occupancy 1.0 / 0.4 by quadrant, density_thresh 0.5: a device mean of 0.25 decides (every pixel covered), one of 0.75 does
    not (the 1.0 quadrants only), and N == 0 writes a count of 0 and nothing else."""
    from radnerf import train_torso
    m = _train_scene(8).model
    N = 1025
    gen = _gen(41)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    xy = _pixels(mask, gen)
    grid = _quadrants() + 0.4 * (1 - _quadrants())
    with _occupancy(m, grid):
        for mean, n_want in ((0.25, N), (0.75, int(mask.sum()))):
            m._mean_density_torso_dev = torch.tensor([mean], dtype=torch.float32, device="cuda")
            idx = _check_select(m, xy, min(THRESH, mean), f"mean {mean}")
            assert idx.numel() == n_want, (mean, idx.numel(), n_want)
        gd = _Guard()
        covered, xy_c, count = train_torso.select(m, xy[:0], alloc=gd.new)
        gd.check()
        assert covered.shape == (0,) and xy_c.shape == (0, 2) and int(count[0]) == 0


# ================================================================================================================== loss
def _entropy(a):
    a = a.clamp(1e-5, 1 - 1e-5)
    return -a * torch.log2(a) - (1 - a) * torch.log2(1 - a)


def _loss_of(alpha_c, color_c, idx, bg, target):
    """The torso loss of Trainer.train_step as PyTorch states it today (index_copy, blend, MSE, entropy), in the inputs' dtype."""
    N = bg.shape[0]
    alpha = torch.zeros(N, 1, dtype=bg.dtype, device=bg.device).index_copy(0, idx, alpha_c)
    color = torch.zeros(N, 3, dtype=bg.dtype, device=bg.device).index_copy(0, idx, color_c)
    pred = color * alpha + bg * (1 - alpha)
    loss = torch.nn.functional.mse_loss(pred, target, reduction="none").mean(-1).mean() + 1e-4 * _entropy(alpha).mean()
    return loss, pred, alpha


LOSS_CASES = [(1, "half"), (65, "half"), (1025, "half"), (4097, "half"), (1025, "none"), (1025, "all")]


@pytest.mark.parametrize("N,cover", LOSS_CASES)
def test_loss_kernel_against_float64(hiplib, N, cover):
    """loss, pred, alpha_full and the gradients of the live compact rows against the float64 restatement, the fp32 PyTorch
    expression as yardstick.  Alphas exactly 0, below 1e-5 and above 1 - 1e-5 sit among the live rows (the clamp hands no entropy
    gradient on); compact rows past the count hold NaN / pixel 0 and must be neither read nor written; uncovered pred == bg."""
    from radnerf import train_torso
    gen = _gen(500 + N)
    r = lambda *s: torch.rand(*s, device="cuda", generator=gen)  # noqa: E731
    mask = {"half": r(N) < 0.5, "none": torch.zeros(N, dtype=torch.bool, device="cuda"), "all": torch.ones(N, dtype=torch.bool, device="cuda")}[cover]
    idx = torch.nonzero(mask).reshape(-1)
    k = idx.numel()
    bg, target = r(N, 3), r(N, 3)
    alpha_live, color_live = r(k, 1) * 0.98 + 0.01, r(k, 3)
    for j, v in enumerate((0.0, 5e-6, 1 - 5e-6, 1.0)):
        if 4 * j + 3 < k:
            alpha_live[4 * j + 3] = v
    alpha_c = torch.full((N, 1), float("nan"), device="cuda")
    color_c = torch.full((N, 3), float("nan"), device="cuda")
    alpha_c[:k], color_c[:k] = alpha_live, color_live
    covered = torch.zeros(N, dtype=torch.int32, device="cuda")          # rows past the count name pixel 0: they must not count
    covered[:k] = idx.int()
    count = torch.tensor([k], dtype=torch.int32, device="cuda")

    runs = {}
    for name, dt in (("f64", torch.float64), ("torch", torch.float32)):
        a, c = alpha_live.clone().to(dt).requires_grad_(True), color_live.clone().to(dt).requires_grad_(True)
        loss, pred, alpha = _loss_of(a, c, idx, bg.to(dt), target.to(dt))
        out = {"loss": loss.detach(), "pred": pred.detach()}
        if k:
            g = torch.autograd.grad(loss, [a, c])
            out.update(alpha_full=alpha.detach(), g_alpha_c=g[0], g_color_c=g[1])
        runs[name] = out

    gd = _Guard()
    loss, pred, alpha_full = train_torso.torso_loss(alpha_c.requires_grad_(True), color_c.requires_grad_(True), covered, count, bg, target,
                                                    alloc=gd.new)
    gd.check()
    (g_alpha, g_color) = loss._rn_direct[1]
    assert loss.shape == () and pred.shape == (N, 3) and alpha_full.shape == (N, 1) and g_alpha.shape == (N, 1) and g_color.shape == (N, 3)
    assert bool((g_alpha[k:] == INSIDE).all()) and bool((g_color[k:] == INSIDE).all()), "gradient rows past the count were written"
    un = ~mask
    assert torch.equal(pred[un], bg[un]) and int(torch.count_nonzero(alpha_full[un])) == 0
    assert torch.equal(alpha_full[idx], alpha_live)
    got = {"loss": loss.detach(), "pred": pred}
    if k:
        got.update(alpha_full=alpha_full, g_alpha_c=g_alpha[:k], g_color_c=g_color[:k])
        flat = (alpha_live.reshape(-1) < 1e-5) | (alpha_live.reshape(-1) > 1 - 1e-5)
        if k > 15:
            assert int(flat.sum()) == 4
        # outside the clamp only the blend's share of d loss / d alpha is left
        blend = ((color_live - bg[idx]) * 2 * (pred[idx] - target[idx]) / (3 * N)).sum(-1)
        if bool(flat.any()):                      # an entropy term there would be 3e-3 of the blend's
            assert float((g_alpha[:k].reshape(-1)[flat] - blend[flat]).abs().max()) <= 1e-5 * float(blend.abs().max())
    for key in got:
        print(f"torso loss N={N} {cover} {key}: e_kernel {_maxerr(got[key], runs['f64'][key]):.3e}  e_torch {_maxerr(runs['torch'][key], runs['f64'][key]):.3e}")
    _compare(got, runs["torch"], runs["f64"], f"torso loss N={N} {cover}")
    # the ready-made gradients reach autograd as they are
    from radnerf import train_head
    train_head.backward(loss)
    assert torch.equal(alpha_c.grad[:k], g_alpha[:k]) and torch.equal(color_c.grad[:k], g_color[:k])


def test_loss_refuses_a_background_that_wants_a_gradient(hiplib):
    from radnerf import train_torso
    z = torch.zeros(4, 3, device="cuda")
    with pytest.raises(ValueError, match="background"):
        train_torso.torso_loss(z[:, :1], z, torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                               z.clone().requires_grad_(True), z)


# ================================================================================================== the layer in a step
def _batch(scene, xy, bg, target, poses):
    """A loader batch (the keys of train_step) of N arbitrary rays of frame 0 whose background pixels are the test's own."""
    N = xy.shape[0]
    f = scene.frame(0)
    pick = torch.randint(0, f["rays_o"].shape[1], (N,), device="cuda", generator=_gen(N))
    return dict(rays_o=f["rays_o"][:, pick].contiguous(), rays_d=f["rays_d"][:, pick].contiguous(), bg_coords=xy.view(1, N, 2), poses=poses,
                face_mask=torch.zeros(1, N, dtype=torch.bool, device="cuda"), eye=f["eye"], auds=f["auds"], index=[ROW],
                bg_color=bg.view(1, N, 3), bg_torso_color=target.view(1, N, 3), images=target.view(1, N, 3))


def _train_step(m, opt, data):
    from radnerf.train import _backward, train_step
    for p in m.parameters():
        p.grad = None
    with _spy() as called:
        pred, _, loss = train_step(m, data, opt)
        _backward(loss)
    return pred, loss, called


PER_OP = ("rn_torso_mask", "rn_mlp64_", "rn_freq_encode", "rn_grid_encode")


@pytest.mark.parametrize("N", [65, 4097])
def test_layer_on_a_live_count(hiplib, monkeypatch, N):
    """train_step's torso route with the opt-in on a half-covered batch of smooth pixels: loss, prediction, all seven parameter
    gradients and the picked code row against float64, the default path under RN_MLP_TRAIN=torch as yardstick; select and the
    loss kernel once each and nothing of the per-operator path."""
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    gen = _gen(7100 + N)
    mask = torch.rand(N, device="cuda", generator=gen) < 0.5
    idx = torch.nonzero(mask).reshape(-1)
    xy = _pixels(mask, gen)
    xy[idx], _ = _smooth_batch(m, idx.numel(), 7101 + N, poses, _code(m, ROW), inside=True)
    bg, target = torch.rand(N, 3, device="cuda", generator=gen), torch.rand(N, 3, device="cuda", generator=gen)
    data = _batch(scene, xy, bg, target, poses)
    with _occupancy(m, _quadrants()):
        ref = netref64.Net64(m)
        a, c, _ = ref.forward_torso(xy[idx], poses, ref.P["individual_codes_torso"][ROW])
        loss64, pred64, alpha64 = _loss_of(a, c, idx, bg.double(), target.double())
        g64 = dict(zip(names, torch.autograd.grad(loss64, [ref.P[n] for n in names])))
        g64["individual_codes_torso"] = g64["individual_codes_torso"][ROW]
        g64.update({"out:loss": loss64.detach(), "out:pred": pred64.detach()})
        runs = {}
        for mode in ("default", "resident"):
            _env(monkeypatch, fused=mode == "resident", mlp="torch" if mode == "default" else None)
            pred, loss, called = _train_step(m, scene.opt, data)
            if mode == "resident":
                assert called.count("rn_torso_select") == 1 and called.count("rn_train_torso_loss") == 1, called
                assert not [c for c in called if c.startswith(PER_OP)], called
                alpha_full = loss._rn_torso_alpha
                assert torch.equal(alpha_full.reshape(-1) > 0, mask) and torch.equal(pred[~mask], bg[~mask])
                assert _maxerr(alpha_full, alpha64) <= 3e-5
            else:
                assert "rn_torso_select" not in called and called.count("rn_torso_mask") == 1, called
            runs[mode] = dict(_collect(m, names, ROW), **{"out:loss": loss.detach(), "out:pred": pred.detach()})
    _compare(runs["resident"], runs["default"], g64, f"torso step N={N}")


def test_layer_with_no_covered_pixel(hiplib, monkeypatch):
    """A device count of 0 at a capacity of 65 rows: every weight gradient, the table's and the codes' exactly zero, the
    prediction the background and the loss the background's."""
    scene = _train_scene(8)
    m, poses = scene.model, _poses(scene)
    names = _grad_names(m)
    N = 65
    gen = _gen(7300)
    xy = _pixels(torch.zeros(N, dtype=torch.bool, device="cuda"), gen)
    bg, target = torch.rand(N, 3, device="cuda", generator=gen), torch.rand(N, 3, device="cuda", generator=gen)
    _env(monkeypatch, fused=True)
    with _occupancy(m, _quadrants()):
        pred, loss, called = _train_step(m, scene.opt, _batch(scene, xy, bg, target, poses))
    assert called.count("rn_torso_select") == 1 and called.count("rn_train_torso_forward") == 1 and called.count("rn_train_torso_loss") == 1
    params = dict(m.named_parameters())
    for n in names:
        g = params[n].grad
        assert g is not None and g.shape == params[n].shape and int(torch.count_nonzero(g)) == 0, n
    assert torch.equal(pred, bg)
    want = ((bg.double() - target.double()) ** 2).mean(-1).mean() + 1e-4 * _entropy(torch.zeros(1, dtype=torch.float64, device="cuda"))[0]
    assert abs(float(loss) - float(want)) <= 1e-6 * float(want)


# ======================================================================================================== whole steps
def _torso_training(size, seed=21):
    """A scene with the torso, its 2-D occupancy set by quadrant to 1.0 / 0.004 around the threshold of 0.01 (mean 0.5: the
    threshold decides, half of the image is covered), a stream whose target is the scene's own render, and the torso net's last
    layer knocked off that target."""
    from radnerf.scene import SyntheticScene, default_opt
    from radnerf.train import SyntheticTrainStream
    torch.manual_seed(seed)
    scene = SyntheticScene(H=size, W=size, n_frames=8, device="cuda", opt=default_opt(engine="ops", torso=True, smooth_lips=False))
    m = scene.model
    m.density_grid_torso.copy_((_quadrants() + 0.004 * (1 - _quadrants())).reshape(-1))
    m.mean_density_torso = 0.5
    stream = SyntheticTrainStream(scene, n_rays=2048, seed=4)
    with torch.no_grad():
        w = m.torso_net.net[-1].weight
        w.add_(0.5 * torch.randn_like(w))
    return scene, stream


@contextlib.contextmanager
def _sync_is_an_error():
    keep = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode(keep)


def test_step_makes_no_host_sync(hiplib, monkeypatch):
    """Whole Trainer.step()s of the device-resident route under torch.cuda.set_sync_debug_mode("error"), with the mean density in
    device memory (after an occupancy refresh) and set from the host; the default path in the same mode is stopped at its
    first read-back (mean_density_torso.item(), then torch.nonzero), which shows that the mode -- a prototype, torch warns -- sees
    what it is meant to see on this build.  The capture in test_captured_step is the second check: it raises on any sync."""
    from radnerf.train import Trainer
    scene, stream = _torso_training(32)
    m = scene.model
    trainer = Trainer(m, scene.opt, update_extra_interval=0)
    _env(monkeypatch, fused=True)
    losses = [trainer.step(stream.batch())]                  # first window: the marcher reads its sample count back
    m.mean_count = 20000
    losses += [trainer.step(stream.batch()) for _ in range(2)]            # caches warm: index tensor, workspaces, learning rates
    batches = [stream.batch() for _ in range(3)]
    with _sync_is_an_error(), _spy() as called:
        losses.append(trainer.step(batches[0]))
    assert called.count("rn_torso_select") == 1 and called.count("rn_train_torso_loss") == 1 and "rn_torso_mask" not in called, called
    with torch.no_grad():
        m.update_extra_state()                               # the refresh leaves the mean on the device
    assert m._mean_density_torso_dev is not None
    with _sync_is_an_error():
        losses.append(trainer.step(batches[1]))
    assert m._mean_density_torso_dev is not None             # nobody asked the host for it
    _env(monkeypatch, fused=False)
    with _sync_is_an_error(), pytest.raises(RuntimeError, match="synchroniz"):
        trainer.step(batches[2])
    assert all(np.isfinite(float(v)) for v in losses)


def test_captured_step(hiplib, monkeypatch):
    """15 steps of torso training: the default path under RN_MLP_TRAIN=torch and =hip, the device-resident route eager, and the
    same replayed from a graph (3 eager steps of the first window, one capture, 12 replays).  Graphed against eager: the project's
    bar for that comparison, rtol 1e-2.  Device-resident against default: max(1e-2, 4 x the gap between the two default curves).
    Every curve falls.  Then the mean density in device memory is lowered under the threshold between two replays of the same
    batch: the second covers every pixel, without a new capture."""
    from radnerf import occupancy
    from radnerf.train import GraphedTrainer, Trainer
    curves = {}
    for kind in ("torch", "hip", "resident", "graph"):
        _env(monkeypatch, fused=kind in ("resident", "graph"), mlp=kind if kind in ("torch", "hip") else None)
        scene, stream = _torso_training(64)
        m = scene.model
        trainer = (GraphedTrainer if kind == "graph" else Trainer)(m, scene.opt, lr_net=5e-3, update_extra_interval=0)
        losses = []
        for i in range(15):
            if i == 3:
                m.mean_count = 40000
                torch.manual_seed(22)
            losses.append(float(trainer.step(stream.batch())))
        curves[kind] = np.array(losses)
    print("torso step curves", {k: v.tolist() for k, v in curves.items()})
    assert trainer.captures == 1 and trainer.replays == 12
    for kind, v in curves.items():
        assert np.isfinite(v).all() and v[14] < v[0], (kind, v)
    np.testing.assert_allclose(curves["graph"], curves["resident"], rtol=1e-2, atol=1e-7)
    gap = float((np.abs(curves["hip"] - curves["torch"]) / curves["torch"]).max())
    bar = max(1e-2, 4 * gap)
    off = float((np.abs(curves["resident"] - curves["torch"]) / curves["torch"]).max())
    print(f"torso step: default hip vs torch {gap:.3e}, device-resident vs default {off:.3e} (bar {bar:.3e})")
    assert off <= bar, (off, bar)

    # the graph reads the mean density when it runs
    b = stream.batch()
    n = b["bg_coords"].shape[1]
    half = occupancy.torso_pixels(m, b["bg_coords"].reshape(-1, 2), m.density_thresh_torso).numel()
    assert 0 < half < n
    trainer.step(b)
    alpha = trainer._plain.newest()[1]._rn_torso_alpha
    assert int((alpha > 0).sum()) == half
    assert m._mean_density_torso_dev is not None
    m._mean_density_torso_dev.fill_(0.001)                   # under every cell of the grid
    trainer.step(b)
    assert int((alpha > 0).sum()) == n
    assert trainer.captures == 1 and trainer.replays == 14
