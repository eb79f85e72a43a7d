"""NeRFNetwork.forward_torso under autograd as one forward and one backward kernel (csrc/rn_train_torso.hip, C ABI
include/radnerf_train.h).

Reference: NeRFNetwork.forward_torso (nerf/network.py:188-219) on the covered pixels of a training batch, differentiated by
torch.autograd in Trainer.train_step.  One call of `torso_forward` is 2 launches (weight image + the layer), its backward 6
(the layer, weight gradients + reduction + constant columns, the memset of the table gradient and its scatter) -- against two
frequency encodes, the grid operator, two MLP stacks of five launches each, pads, concatenations and the autograd of all of it.
Differentiable in the six weight matrices, the torso table and the individual code; the pixel coordinates get no gradient.

Opt-in: RN_TORSO_TRAIN=fused in the environment.  Eager, on the caller's stream.
"""
import ctypes as C
import os

import torch

import radnerf_hip as hip
from radnerf_hip.abi import TorsoGradsT

from .fused import _grid_desc, torso_constants, torso_weights, torso_weights_desc  # noqa: F401  (torso_weights: re-exported)
from .train_head import grid_scatter

_lib = hip._lib


def supported(model):
    """The network shape the kernels are built for (= the fused inference engine's, with the torso), an fp32 torso table,
    linear interpolation, align_corners off."""
    from . import fused
    try:
        enc = model.torso_encoder if model.torso else None
        return bool(model.torso and fused.supported(model) and enc.embeddings.dtype == torch.float32 and enc.input_dim == 2
                    and enc.interp_id == 0 and not enc.align_corners and float(model.opt.torso_shrink) > 0)
    except AttributeError:
        return False


def usable(model, x):
    """Opted in (RN_TORSO_TRAIN=fused) and a training call of the supported shape on the GPU in fp32; autocast, no_grad and
    anything else keep the per-operator path."""
    return (os.environ.get("RN_TORSO_TRAIN") == "fused" and x.is_cuda and torch.is_grad_enabled() and x.dim() == 2
            and x.dtype == torch.float32 and not torch.is_autocast_enabled() and supported(model))


def _empty(dev):
    def alloc(*shape):
        return torch.empty(*shape, dtype=torch.float32, device=dev)
    return alloc


class _TorsoTrain(torch.autograd.Function):
    """(alpha [P,1], color [P,3], dx [P,2]) = NeRFNetwork.forward_torso(xy, poses, None, code).  meta = (torso_encoder,
    torso_shrink, alloc): alloc(*shape) hands out every buffer the kernels write results into (None: torch.empty)."""

    @staticmethod
    def forward(ctx, xy, poses, code, p_dev, meta, table, *ws):
        enc, shrink, alloc = meta
        dev = xy.device
        alloc = alloc or _empty(dev)
        P = xy.shape[0]
        xy = xy.detach().contiguous()
        ws = [w.detach().contiguous() for w in ws]
        ind_dim = ws[0].shape[1] - 96
        assert xy.shape[1] == 2
        p6, code_c = torso_constants(poses, code if ind_dim else None)
        assert p6.numel() == 6 and (code_c is None or code_c.numel() == ind_dim)
        tab = hip.aligned(table.detach(), 64)
        tw = torso_weights_desc(ws, ind_dim)
        gd = _grid_desc(enc, tab)
        s = hip.stream()
        alpha, color, dx, wn = alloc(P, 1), alloc(P, 3), alloc(P, 2), alloc(P, 2)
        image = work = None
        if P:
            image = torch.empty(int(_lib.rn_train_torso_image_floats()), dtype=torch.float32, device=dev)
            work = torch.empty(int(_lib.rn_train_torso_workspace_floats(P)), dtype=torch.float32, device=dev)
            hip.call("rn_train_torso_pack", C.byref(tw), hip.ptr(p6), hip.ptr(code_c), hip.ptr(image), s)
            hip.call("rn_train_torso_forward", hip.ptr(xy), P, hip.ptr(p_dev), float(shrink), C.byref(gd), hip.ptr(image), hip.ptr(alpha),
                     hip.ptr(color), hip.ptr(dx), hip.ptr(wn), hip.ptr(work), s)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(xy, code_c, p_dev, tab, image, work, alpha, color, wn, *ws)
        ctx.meta = (enc, float(shrink), alloc, P, ind_dim, None if code is None else code.shape)
        return alpha, color, dx

    @staticmethod
    def backward(ctx, g_alpha, g_color, g_dx):
        xy, code_c, p_dev, tab, image, work, alpha, color, wn, *ws = ctx.saved_tensors
        enc, shrink, alloc, P, ind_dim, code_shape = ctx.meta
        dev = xy.device
        s = hip.stream()

        def dense(g):
            if g is None:
                return None
            g = g.contiguous()
            return g if g.dtype == torch.float32 else g.float()
        g_alpha, g_color, g_dx = dense(g_alpha), dense(g_color), dense(g_dx)
        grads = [alloc(*w.shape) for w in ws]
        g_code = alloc(ind_dim) if ind_dim else None
        if P:
            g_feat = alloc(16 * P, 2)
            hip.call("rn_train_torso_backward", hip.ptr(g_alpha), hip.ptr(g_color), hip.ptr(g_dx), hip.ptr(alpha), hip.ptr(color), P,
                     hip.ptr(p_dev), hip.ptr(image), hip.ptr(work), hip.ptr(g_feat), s)
            tw = torso_weights_desc(ws, ind_dim)
            tg = TorsoGradsT()
            (tg.def_w0, tg.def_w1, tg.def_w2, tg.tor_w0, tg.tor_w1, tg.tor_w2) = [g.data_ptr() for g in grads]
            tg.ind_code = hip.ptr(g_code)
            wsp = hip.workspace(int(_lib.rn_train_torso_wgrad_workspace()), dev)
            hip.call("rn_train_torso_weight_grads", C.byref(tw), hip.ptr(xy), shrink, hip.ptr(code_c), P, hip.ptr(p_dev), hip.ptr(image),
                     hip.ptr(work), C.byref(tg), hip.ptr(wsp), s)
            g_table = torch.zeros_like(tab)
            grid_scatter([(g_feat, wn, enc, _grid_desc(enc, tab), g_table)], P, p_dev)
        else:
            g_table = torch.zeros_like(tab)
            for g in grads:
                g.zero_()
            if g_code is not None:
                g_code.zero_()
        return (None, None, g_code.view(code_shape) if g_code is not None else None, None, None, g_table, *grads)


def torso_forward(model, xy, poses, code, p_dev=None, alloc=None):
    """-> (alpha [P,1], color [P,3], dx [P,2]) through the fused training kernels.  xy [P,2] in [-1, 1], poses [1,6], code: the
    individual code [ind_dim] (an autograd index of individual_codes_torso stays with the caller) or None.  p_dev: optional int32
    device scalar, the number of live pixel rows.  alloc: see _TorsoTrain."""
    ws = torso_weights(model)
    if model.individual_dim_torso == 0:
        code = None
    elif code is None:
        raise ValueError("torso_forward: this model has an individual code for the torso; pass it")
    return _TorsoTrain.apply(xy, poses, code, p_dev, (model.torso_encoder, float(model.opt.torso_shrink), alloc),
                             model.torso_encoder.embeddings, *ws)
