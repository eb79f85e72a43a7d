"""NeRFNetwork.forward_torso under autograd as one forward and one backward kernel (csrc/rn_train_torso.hip, C ABI
include/radnerf_train.h).

Reference: NeRFNetwork.forward_torso (nerf/network.py:188-219) on the covered pixels of a training batch, differentiated by
torch.autograd in Trainer.train_step.  One call of `torso_forward` is 2 launches (weight image + the layer), its backward 6
(the layer, weight gradients + reduction + constant columns, the memset of the table gradient and its scatter) -- against two
frequency encodes, the grid operator, two MLP stacks of five launches each, pads, concatenations and the autograd of all of it.
Differentiable in the six weight matrices, the torso table and the individual code; the pixel coordinates get no gradient.

Opt-in: RN_TORSO_TRAIN=fused in the environment.  On the caller's stream.

With the opt-in a training step (radnerf/train.py: train_step) keeps the whole torso part on the device: `select` compacts the
covered pixels of the batch in ascending order and leaves their count in device memory (rn_torso_select, csrc/rn_torso.hip),
`torso_forward` runs at the capacity of all N rows with that count as its live count, and `torso_loss` scatters back, blends over
the background and takes MSE + entropy with their gradients in one launch (rn_train_torso_loss) -- no torch.nonzero, no .item(),
no shape that depends on the data, so GraphedTrainer can capture the step.  RN_TORSO_STEP=host keeps the fused layer on the index
list the host asks for (rn_torso_mask + torch.nonzero), for comparisons.
"""
import ctypes as C

import torch

import radnerf_hip as hip
from radnerf_hip.abi import TorsoGradsT

from . import switches
from .fused import _grid_desc, torso_constants, torso_weights, torso_weights_desc  # noqa: F401  (torso_weights: re-exported)
from .route import training_call
from .train_head import grid_scatter, prepare_scatter

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
    return switches.get("RN_TORSO_TRAIN") == "fused" and training_call(x) and x.dim() == 2 and supported(model)


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
            wsp = _wgrad_workspace(dev)
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


def step_enabled():
    """Is the device-resident torso step switched on?  RN_TORSO_TRAIN=fused, and not RN_TORSO_STEP=host: the fused layer on the
    index list the host asks for (rn_torso_mask + torch.nonzero), for comparisons."""
    return switches.get("RN_TORSO_TRAIN") == "fused" and switches.get("RN_TORSO_STEP") == "device"


def step_usable(model, bg_coords, background, target=None):
    """May a training step take the device-resident route (select -> torso_forward on a live count -> torso_loss)?  Opted in, the
    supported shape, fp32 CUDA tensors, no autocast, grad enabled, and a background that is a tensor without a gradient (the loss
    kernel returns none for it)."""
    tensors = [bg_coords, background] + ([target] if target is not None else [])
    return (step_enabled() and model.training and all(torch.is_tensor(t) for t in tensors) and training_call(*tensors)
            and not background.requires_grad and supported(model))


def pin_mean(model):
    """The mean torso density as a device scalar at ONE fixed address, whatever set it last -- the occupancy refresh's own
    `stats_torso`: the refresh leaves it there; a value set from the host (checkpoint, the setter) or held in another tensor is
    written into that buffer.  Call outside a capture: a captured select reads the buffer at every replay."""
    from . import occupancy
    stats = occupancy._scratch(model).stats_torso
    held = model._mean_density_torso_dev
    if held is None:
        stats.fill_(float(model._mean_density_torso))
    elif held is not stats:
        stats.copy_(held.reshape(-1)[:1])
    model._mean_density_torso_dev = stats
    return stats


def _wgrad_workspace(dev):
    """The weight-gradient scratch of the torso layer: its own buffer per device, of the one size the library asks for.  It never
    grows and nothing else uses it, so a captured step can keep its address (the shared hip.workspace() buffer is replaced when a
    larger request comes); prepare() creates it before a capture."""
    return hip.persistent_buffer("train_torso.wgrad", int(_lib.rn_train_torso_wgrad_workspace()), dev)


def prepare(model, n_px):
    """Everything persistent a captured torso step of `n_px` pixels touches, created before the capture: the pinned mean density,
    the weight-gradient workspace, the host copy of the table's level offsets, and with RN_TRAIN_DETERMINISTIC=1 the ordered table
    scatter's workspace (the layer runs at the capacity of all n_px rows)."""
    dev = model.density_grid_torso.device
    pin_mean(model)
    _wgrad_workspace(dev)
    hip.host_offsets(model.torso_encoder.offsets)
    prepare_scatter((model.torso_encoder,), n_px, dev)


def select(model, bg_coords, alloc=None):
    """-> (covered int32 [N], xy_c [N,2], count int32 [1]): the pixels of bg_coords [N,2] the torso layer covers (ascending, the
    order of occupancy.torso_pixels) and their coordinates, compacted on the device; rows at or past `count` are not written.
    The threshold min(density_thresh_torso, mean_density_torso) takes the mean from device memory while the refresh's value is
    still there, so nothing here waits for the GPU."""
    N, dev = int(bg_coords.shape[0]), bg_coords.device
    coords = bg_coords.contiguous()
    mean = model._mean_density_torso_dev
    thresh = float(model.density_thresh_torso) if mean is not None else min(model.density_thresh_torso, model._mean_density_torso)
    if alloc is None:
        covered = torch.empty(N, dtype=torch.int32, device=dev)
        xy_c = torch.empty(N, 2, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
    else:
        covered, xy_c, count = alloc(N, dtype=torch.int32), alloc(N, 2), alloc(1, dtype=torch.int32)
    hip.call("rn_torso_select", hip.ptr(coords, torch.float32), N, hip.ptr(model.density_grid_torso), int(model.grid_size), float(thresh),
             hip.ptr(mean), hip.ptr(covered), hip.ptr(xy_c), hip.ptr(count), hip.stream())
    return covered, xy_c, count


class _TorsoLoss(torch.autograd.Function):
    """Scatter-back, blend, MSE + entropy of a torso step in one kernel; returns (loss, pred, alpha_full, gradients)."""

    @staticmethod
    def forward(ctx, alpha_c, color_c, covered, count, bg, target, alloc):
        P, N, dev = alpha_c.shape[0], bg.shape[0], bg.device
        alpha_c, color_c = alpha_c.contiguous(), color_c.contiguous()
        if alloc is None:
            out = torch.empty(4 * N + 4 * P + 1, dtype=torch.float32, device=dev)
            pred, alpha_full = out[0:3 * N].view(N, 3), out[3 * N:4 * N].view(N, 1)
            grads, loss = out[4 * N:4 * N + 4 * P], out[4 * N + 4 * P:]
        else:
            pred, alpha_full, grads, loss = alloc(N, 3), alloc(N, 1), alloc(4 * P), alloc(1)
        g_alpha, g_color = grads[0:P].view(P, 1), grads[P:4 * P].view(P, 3)
        hip.call("rn_train_torso_loss", hip.ptr(alpha_c), hip.ptr(color_c), hip.ptr(covered), P, hip.ptr(count), bg.data_ptr(), bg.stride(0),
                 target.data_ptr(), target.stride(0), N, loss.data_ptr(), pred.data_ptr(), alpha_full.data_ptr(), g_alpha.data_ptr(),
                 g_color.data_ptr(), hip.stream())
        ctx.save_for_backward(grads)
        ctx.P = P
        ctx.mark_non_differentiable(pred, alpha_full, grads)
        ctx.set_materialize_grads(False)
        return loss.view(()), pred, alpha_full, grads

    @staticmethod
    def backward(ctx, g, *_unused):
        (grads,) = ctx.saved_tensors
        P = ctx.P
        if g is None:
            return (None,) * 7
        scaled = grads * g                        # rows past the live count hold nothing; the layer's backward never reads them
        return scaled[0:P].view(P, 1), scaled[P:4 * P].view(P, 3), None, None, None, None, None


def torso_loss(alpha_c, color_c, covered, count, bg, target, alloc=None):
    """The torso loss of Trainer.train_step from the compact rows of the layer: alpha_c [P,1], color_c [P,3] (rows below `count`
    live), covered int32 [P] ascending, count int32 [1] on the device, bg / target [N,3] fp32 (rows may be strided views of one
    batch table; bg gets no gradient).  -> (loss, pred [N,3] = results["torso_color"], alpha_full [N,1] = results["torso_alpha"])."""
    def rows(t):
        t = t.reshape(-1, 3)
        return t if t.stride(1) == 1 and t.stride(0) >= 3 else t.contiguous()
    if bg.requires_grad:
        raise ValueError("torso_loss: the background gets no gradient from this kernel; take the per-operator path")
    bg, target = rows(bg), rows(target)
    if bg.shape[0] != target.shape[0] or alpha_c.shape[0] > bg.shape[0]:
        raise ValueError(f"torso_loss: {bg.shape[0]} background rows, {target.shape[0]} target rows, {alpha_c.shape[0]} compact rows")
    loss, pred, alpha_full, grads = _TorsoLoss.apply(alpha_c, color_c, covered, count, bg, target, alloc)
    loss._rn_torso_alpha = alpha_full            # what results["torso_alpha"] holds; a captured step keeps it with its loss
    # d loss / d (alpha_c, color_c) were written by the same kernel: train_head.backward(loss) hands them to autograd as they are
    P = alpha_c.shape[0]
    loss._rn_direct = ((alpha_c, color_c), (grads[0:P].view(P, 1), grads[P:4 * P].view(P, 3)))
    return loss, pred, alpha_full


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
