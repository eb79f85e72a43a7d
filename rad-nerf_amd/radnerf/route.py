"""What the routes through a training step share, without the HIP library: the predicate for a training call, and the
table-gradient scatters a backward pass leaves running for the optimizer to join."""
import contextlib
import functools
import importlib

import torch


def training_call(*tensors):
    """Grad enabled, autocast off, every tensor fp32 on the device: what every training kernel asks of its call (each caller adds
    what is its own: a rank, a row threshold, the model's shape)."""
    return (torch.is_grad_enabled() and not torch.is_autocast_enabled()
            and all(t.is_cuda and t.dtype == torch.float32 for t in tensors))


@functools.lru_cache(maxsize=None)
def kernels(name):
    """radnerf.<name>, one of the modules over the HIP library: imported when a route first asks for it, never on the CPU path."""
    return importlib.import_module("." + name, __package__)


DEFER_JOIN = False      # inside deferred_join(): the optimizer waits for take_pending_events() (radnerf.train.Trainer with HipAdam)
_PENDING = []


@contextlib.contextmanager
def deferred_join():
    """with deferred_join(): ... loss.backward(); optimizer.step() -- the optimizer (HipAdam.step) joins the side stream."""
    global DEFER_JOIN
    prev, DEFER_JOIN = DEFER_JOIN, True
    try:
        yield
    finally:
        DEFER_JOIN = prev


def take_pending_events():
    """(event, gradient addresses...) of table-gradient scatters still running on the side stream (RN_TRAIN_OVERLAP=1): whoever
    reads the table gradients next (the optimizer) makes its stream wait for them."""
    evs = list(_PENDING)
    _PENDING.clear()
    return evs
