"""What the GPU tests of the fused training head share (tests/test_gpu_train_head_f16.py: RN_TRAIN_MLP=f16 against the
arithmetic model netref16; tests/test_gpu_train_head_ref.py: the default fp32 route against float64): the seeded models, the
picked batches, one run of the head through the C ABI on sentinel-filled buffers (`direct`, `weight_grads`), one through
autograd (`head`), the plain fp32 formulation of the same network (`ops`) and the float64 reference in chunks of rows
(`reference64`)."""
import ctypes as C
import os

import torch

import headref32
import netref16
from netref64 import Net64Libm

_SCENES, _BATCHES, _BATCHES32 = {}, {}, {}


def model(tag):
    if tag not in _SCENES:
        _SCENES[tag] = netref16.head_scene(tag, "cuda")
    m = _SCENES[tag].model
    m.train()
    return m


def batch(tag, M, seed):
    """netref16.stable_batch, once per (model, size, seed): the tests share it and leave it unchanged."""
    key = (tag, M, seed)
    if key not in _BATCHES:
        _BATCHES[key] = netref16.stable_batch(netref16.Net16(model(tag)), M, seed)
    return _BATCHES[key]


def batch32(tag, M, seed):
    """headref32.stable_batch32, once per (model, size, seed): the tests share it and leave it unchanged."""
    key = (tag, M, seed)
    if key not in _BATCHES32:
        _BATCHES32[key] = headref32.stable_batch32(Net64Libm(model(tag)), M, seed)
    return _BATCHES32[key]


def environment(monkeypatch, mlp, deterministic=False):
    monkeypatch.setenv("RN_TRAIN_HEAD", "fused")
    monkeypatch.setenv("RN_TRAIN_MLP", mlp)
    monkeypatch.setenv("RN_TRAIN_DETERMINISTIC", "1" if deterministic else "0")


def wparts():
    """RN_TRAIN_WPARTS as the library reads it (csrc/rn_train_head.hip: atol of the variable, default 128, clamped to 1 .. 256):
    the workgroups -- partial sums -- per weight-gradient job."""
    text = os.environ.get("RN_TRAIN_WPARTS")
    if text is None:
        return 128
    digits = text.strip()
    end = 1 if digits[:1] in "+-" else 0
    while end < len(digits) and digits[end].isdigit():
        end += 1
    try:
        value = int(digits[:end])
    except ValueError:
        value = 0
    return min(max(value, 1), 256)


def direct(m, b, sfx, M=None, m_dev=None, up=None, sentinel=0.0, ind_row=0):
    """pack + forward (+ backward under `up`) through the C ABI on buffers of this function, every one pre-filled with `sentinel`
    (the workspace with zeros) -> dict of the buffers.  ind_row: the row of individual_codes handed over as the code."""
    import radnerf_hip as hip
    from radnerf.fused import _grid_desc, head_weights, weights_desc
    lib = hip._lib
    M = b["xyzs"].shape[0] if M is None else M
    xyzs, dirs = b["xyzs"][:M].contiguous(), b["dirs"][:M].contiguous()
    ws = [w.detach().contiguous() for w in head_weights(m)]
    audio_dim, has_eye, ind_dim = ws[0].shape[1] - 32, ws[3].shape[1] - 64, ws[6].shape[1] - 80
    enc_a = b["enc_a"].reshape(-1).contiguous()
    eye = b["eye"].reshape(-1).contiguous() if has_eye else None
    ind = m.individual_codes[ind_row].detach().contiguous() if ind_dim else None
    tx, tw = hip.aligned(m.encoder.embeddings.detach(), 64), hip.aligned(m.encoder_ambient.embeddings.detach(), 64)
    nw = weights_desc(ws, audio_dim, has_eye, ind_dim)
    gx, gw = _grid_desc(m.encoder, tx), _grid_desc(m.encoder_ambient, tw)
    s = hip.stream()

    def buf(*shape):
        return torch.full(shape, sentinel, dtype=torch.float32, device="cuda")
    image = torch.zeros(int(getattr(lib, "rn_train_head_image_floats" + sfx)()), dtype=torch.float32, device="cuda")
    hip.call("rn_train_head_pack" + sfx, C.byref(nw), hip.ptr(enc_a), hip.ptr(eye), hip.ptr(ind), hip.ptr(image), s)
    out = dict(image=image, work=torch.zeros(int(lib.rn_train_head_workspace_floats(M)), dtype=torch.float32, device="cuda"),
               sigmas=buf(M), rgbs=buf(M, 3), ambient=buf(M, 2), amb_abs=buf(M), xn=buf(M, 3), wn=buf(M, 2))
    hip.call("rn_train_head_forward" + sfx, hip.ptr(xyzs), hip.ptr(dirs), M, hip.ptr(m_dev), C.byref(gx), C.byref(gw), hip.ptr(image),
             float(m.bound), *(out[k].data_ptr() for k in ("sigmas", "rgbs", "ambient", "amb_abs", "xn", "wn")), hip.ptr(out["work"]), s)
    if up is not None:
        up = [u[:M].contiguous() for u in up]
        out["g_enc_x"], out["g_enc_w"] = buf(16, M, 2), buf(16, M, 2)
        hip.call("rn_train_head_backward" + sfx, hip.ptr(up[0]), hip.ptr(up[1]), hip.ptr(up[3]), hip.ptr(up[2]), out["rgbs"].data_ptr(),
                 out["ambient"].data_ptr(), M, hip.ptr(m_dev), hip.ptr(image), hip.ptr(out["work"]), out["g_enc_x"].data_ptr(),
                 out["g_enc_w"].data_ptr(), s)
    torch.cuda.synchronize()
    return out


def weight_grads(m, b, work, M, ind_row, row_form, sentinel):
    """rn_train_head_weight_grads (the code handed over: individual_codes[ind_row]) or, with row_form, rn_train_head_weight_grads_row
    (the table and the row's index handed over) on the workspace `work` of a `direct` run with backward, every gradient buffer
    pre-filled with `sentinel` -> dict of the buffers; "ind_code" is [ind_dim] or, in row form, the whole table's gradient."""
    import radnerf_hip as hip
    from radnerf.fused import head_weights, weights_desc
    from radnerf_hip.abi import HeadGradsT
    ws = [w.detach().contiguous() for w in head_weights(m)]
    audio_dim, has_eye, ind_dim = ws[0].shape[1] - 32, ws[3].shape[1] - 64, ws[6].shape[1] - 80
    assert ind_dim
    enc_a, eye = b["enc_a"].reshape(-1).contiguous(), (b["eye"].reshape(-1).contiguous() if has_eye else None)
    table = m.individual_codes.detach().contiguous()
    nw = weights_desc(ws, audio_dim, has_eye, ind_dim)

    def buf(*shape):
        return torch.full(shape, sentinel, dtype=torch.float32, device="cuda")
    names = ("amb_w0", "amb_w1", "amb_w2", "sig_w0", "sig_w1", "sig_w2", "col_w0", "col_w1")
    out = {n: buf(*w.shape) for n, w in zip(names, ws)}
    out["enc_a"], out["ind_code"] = buf(audio_dim), (buf(*table.shape) if row_form else buf(ind_dim))
    if has_eye:
        out["eye"] = buf(1)
    hg = HeadGradsT()
    for n in names + ("enc_a", "ind_code"):
        setattr(hg, n, out[n].data_ptr())
    hg.eye = hip.ptr(out.get("eye"))
    wsp = torch.zeros(int(hip._lib.rn_train_head_wgrad_workspace()) // 4, dtype=torch.float32, device="cuda")
    if row_form:
        index = torch.tensor([ind_row], dtype=torch.int64, device="cuda")
        hip.call("rn_train_head_weight_grads_row", C.byref(nw), hip.ptr(enc_a), hip.ptr(eye), hip.ptr(table), hip.ptr(index), int(table.shape[0]),
                 M, None, hip.ptr(work), C.byref(hg), hip.ptr(wsp), hip.stream())
    else:
        code = table[ind_row].contiguous()
        hip.call("rn_train_head_weight_grads", C.byref(nw), hip.ptr(enc_a), hip.ptr(eye), hip.ptr(code), M, None, hip.ptr(work), C.byref(hg),
                 hip.ptr(wsp), hip.stream())
    torch.cuda.synchronize()
    return out


def head(m, b, up, live=None, row=False, input_grads=False, backwards=1):
    """head_forward + backward under head_loss (rows below `live` only, the count handed over on the device) through autograd;
    -> (outputs, [gradients of backward pass i under up * 2^(-20 i)]).  The environment selects the route."""
    from radnerf import train_head
    M = b["xyzs"].shape[0]
    n = M if live is None else live
    enc_a = b["enc_a"].clone().requires_grad_(True)
    eye = b["eye"].clone().requires_grad_(True) if m.exp_eye else None
    xyzs, dirs = b["xyzs"].clone().requires_grad_(input_grads), b["dirs"].clone().requires_grad_(input_grads)
    m_dev = None if live is None else torch.tensor([live, 0], dtype=torch.int32, device="cuda")
    kw = {}
    if m.individual_dim:
        kw = dict(ind_index=torch.tensor([0], dtype=torch.int64, device="cuda")) if row else dict(ind_code=m.individual_codes[0])
    sigma, rgb, amb, amb_abs = train_head.head_forward(m, xyzs, dirs, enc_a, kw.get("ind_code"), eye, m_dev=m_dev, ind_index=kw.get("ind_index"))
    out = {"sigma": sigma.detach()[:n].clone(), "rgb": rgb.detach()[:n].clone(), "ambient": amb.detach()[:n].clone()}
    passes = []
    for i in range(backwards):
        for p in list(m.parameters()) + [enc_a, eye, xyzs, dirs]:
            if p is not None:
                p.grad = None
        u = [t[:n] * 2.0 ** (-20 * i) for t in up]
        loss = (sigma[:n] * u[0]).sum() + (rgb[:n] * u[1]).sum() + (amb_abs[:n] * u[2]).sum() + (amb[:n] * u[3]).sum()
        loss.backward(retain_graph=i + 1 < backwards)
        g = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        g["enc_a"] = enc_a.grad.clone()
        if eye is not None:
            g["eye"] = eye.grad.clone()
        if input_grads:
            g["xyzs"], g["dirs"] = xyzs.grad[:n].clone(), dirs.grad[:n].clone()
        passes.append(g)
    torch.cuda.synchronize()
    return out, passes


def ops(m, b, up, monkeypatch, live=None):
    """The plain fp32 formulation of the same network on the first `live` rows of the batch, under the same upstream gradients:
    NeRFNetwork.forward with RN_TRAIN_HEAD=ops, RN_MLP_TRAIN=torch, RN_TRAIN_GLUE=torch -- nn.Linear / F.relu / tanh / trunc_exp /
    sigmoid / cat / repeat under torch.autograd over the grid and SH operators, none of the head's kernels.  -> (outputs,
    gradients) keyed like head(..., input_grads=True)."""
    monkeypatch.setenv("RN_TRAIN_HEAD", "ops")
    monkeypatch.setenv("RN_MLP_TRAIN", "torch")
    monkeypatch.setenv("RN_TRAIN_GLUE", "torch")
    n = b["xyzs"].shape[0] if live is None else live
    for p in m.parameters():
        p.grad = None
    enc_a = b["enc_a"].clone().requires_grad_(True)
    eye = b["eye"].clone().requires_grad_(True) if m.exp_eye else None
    xyzs, dirs = b["xyzs"][:n].clone().requires_grad_(True), b["dirs"][:n].clone().requires_grad_(True)
    sigma, rgb, amb = m(xyzs, dirs, enc_a, m.individual_codes[0] if m.individual_dim else None, eye)
    netref16.head_loss(sigma, rgb, amb, [u[:n] for u in up]).backward()
    g = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    g["enc_a"], g["xyzs"], g["dirs"] = enc_a.grad.clone(), xyzs.grad.clone(), dirs.grad.clone()
    if eye is not None:
        g["eye"] = eye.grad.clone()
    for p in m.parameters():
        p.grad = None
    torch.cuda.synchronize()
    return {"sigma": sigma.detach(), "rgb": rgb.detach(), "ambient": amb.detach()}, g


def reference64(m, b, up, live=None, chunk=16384):
    """netref16.run_reference(Net64Libm(m): the library's own level scales) with input gradients on the first `live` rows, evaluated `chunk` rows at a time: every
    gradient is linear in the samples, so the parameter and table gradients of the chunks are added (in float64) and the
    per-sample outputs and input gradients concatenated.  One chunk is the plain single pass."""
    n = b["xyzs"].shape[0] if live is None else live
    ref = Net64Libm(m)
    outs, total = [], None
    for at in range(0, n, chunk):
        rows = slice(at, min(at + chunk, n))
        o, g = netref16.run_reference(ref, b["xyzs"][rows], b["dirs"][rows], b["enc_a"], b["eye"], [u[rows] for u in up], input_grads=True)
        outs.append(o)
        if total is None:
            total = {k: ([v] if k in ("xyzs", "dirs") else v.clone()) for k, v in g.items()}
        else:
            for k, v in g.items():
                if k in ("xyzs", "dirs"):
                    total[k].append(v)
                else:
                    total[k] += v
    for k in ("xyzs", "dirs"):
        total[k] = torch.cat(total[k])
    return {k: torch.cat([o[k] for o in outs]) for k in outs[0]}, total
