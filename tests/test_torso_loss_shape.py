"""train_step's torso loss: the prediction is [n, 3] and the loader's target [1, n, 3].  The target is reshaped to the prediction's
shape, so the value is the broadcast one's and mse_loss has no size mismatch to warn about; a target of another size is an error."""
import types
import warnings

import pytest
import torch


class _Model:
    def __init__(self, color, alpha):
        self.out = dict(torso_color=color, torso_alpha=alpha)

    def render(self, *a, **k):
        return self.out


def _data(n, rgb):
    z = torch.zeros(1, n, 3)
    return dict(rays_o=z, rays_d=z, auds=None, bg_coords=torch.zeros(1, n, 2), poses=torch.zeros(1, 6), eye=None, index=[0],
                bg_color=z, face_mask=torch.zeros(1, n, dtype=torch.bool), bg_torso_color=rgb)


OPT = types.SimpleNamespace(torso=True, dt_gamma=0.0, max_steps=16)


def test_torso_loss_value_and_no_broadcast_warning():
    from radnerf.train import entropy_of, train_step
    g = torch.Generator().manual_seed(0)
    n = 37
    color = torch.rand(n, 3, generator=g, dtype=torch.float64).requires_grad_()
    alpha = torch.rand(n, 1, generator=g, dtype=torch.float64)
    rgb = torch.rand(1, n, 3, generator=g, dtype=torch.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # "Using a target size ... different to the input size" would raise
        pred, target, loss = train_step(_Model(color, alpha), _data(n, rgb), OPT)
    assert pred is color and target is rgb                   # what the caller gets back keeps the loader's shape
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # the broadcast form, as the loss was written before
        want = torch.nn.functional.mse_loss(color, rgb, reduction="none").mean(-1).mean() + 1e-4 * entropy_of(alpha).mean()
    assert loss.shape == () and torch.equal(loss, want)      # float64, the same sums in the same order
    g_new, = torch.autograd.grad(loss, color)
    g_old, = torch.autograd.grad(want, color)
    assert g_new.shape == (n, 3) and torch.allclose(g_new, g_old, rtol=0, atol=1e-15)


def test_torso_loss_refuses_a_target_of_another_size():
    from radnerf.train import train_step
    n = 8
    color, alpha = torch.rand(n, 3), torch.rand(n, 1)
    with pytest.raises(RuntimeError):
        train_step(_Model(color, alpha), _data(n, torch.rand(1, 1, 3)), OPT)
