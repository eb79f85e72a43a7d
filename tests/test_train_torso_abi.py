"""rn_train_torso_* (the fused training kernels of the torso layer, include/radnerf_train.h): declared, exported, in the ctypes
table in header order, and refusing bad arguments before anything touches a GPU.  Modelled on tests/test_train_camera_abi.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RN_ERR_INVALID_ARG = -1
ENTRIES = [("rn_train_torso_image_floats", "size_t", 0), ("rn_train_torso_workspace_floats", "size_t", 1),
           ("rn_train_torso_wgrad_workspace", "size_t", 0), ("rn_train_torso_pack", "int", 5), ("rn_train_torso_forward", "int", 12),
           ("rn_train_torso_backward", "int", 11), ("rn_train_torso_weight_grads", "int", 11)]


def test_entries_are_declared_exported_and_in_the_table(hiplib):
    from radnerf_hip import abi
    header = open(os.path.join(ROOT, "include", "radnerf_train.h")).read()
    names = list(abi.FUNCTIONS)
    at = []
    for name, ret, arity in ENTRIES:
        m = re.search(r"\b%s\s+%s\s*\(" % (ret, name), header)
        assert m, f"{name} not declared in include/radnerf_train.h"
        at.append((m.start(), names.index(name)))
        fn = getattr(hiplib._lib, name)                       # AttributeError: the library does not export it
        restype, argtypes = abi.FUNCTIONS[name]
        assert fn.restype is restype and list(fn.argtypes) == argtypes and len(argtypes) == arity, name
        assert restype is (C.c_size_t if ret == "size_t" else C.c_int), name
    assert at == sorted(at) and [i for _, i in at] == sorted(i for _, i in at)        # header order = table order
    assert all(i > names.index("rn_train_batch_gather") for _, i in at)             # after what the header had before


def test_struct_mirror(hiplib):
    from radnerf_hip import abi
    header = open(os.path.join(ROOT, "include", "radnerf_train.h")).read()
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*rn_train_torso_grads_t\s*;", header).group(1)
    fields = re.findall(r"\*\s*(\w+)", body)
    assert fields == ["def_w0", "def_w1", "def_w2", "tor_w0", "tor_w1", "tor_w2", "ind_code"]
    assert abi.TorsoGradsT.c_name == "rn_train_torso_grads_t"
    assert [n for n, _ in abi.TorsoGradsT._fields_] == fields and all(t is C.c_void_p for _, t in abi.TorsoGradsT._fields_)
    assert C.sizeof(abi.TorsoGradsT) == 7 * C.sizeof(C.c_void_p)


def test_sizes(hiplib):
    lib = hiplib._lib
    assert lib.rn_train_torso_image_floats() % 4 == 0 and lib.rn_train_torso_image_floats() > 10320
    per_tile = lib.rn_train_torso_workspace_floats(1)
    assert lib.rn_train_torso_workspace_floats(0) == 0 and per_tile > 0 and per_tile % 4 == 0
    assert lib.rn_train_torso_workspace_floats(32) == per_tile and lib.rn_train_torso_workspace_floats(33) == 2 * per_tile
    assert lib.rn_train_torso_wgrad_workspace() > 6 * 96 * 96 * 4


def test_entries_refuse_bad_arguments(hiplib):
    """Null required pointers, a grid the kernels are not built for (D != 2, L != 16, a non-fp32 table), a misaligned
    feature-gradient pointer and torso_shrink = 0 come back as RN_ERR_INVALID_ARG with a message; P == 0 is a no-op."""
    from radnerf_hip import abi
    lib, err = hiplib._lib, hiplib.last_error
    with open(os.path.join(ROOT, "include", "radnerf_hip.h")) as f:
        assert int(re.search(r"#define\s+RN_ERR_INVALID_ARG\s+\((-?\d+)\)", f.read()).group(1)) == RN_ERR_INVALID_ARG
    # host memory stands in for the device buffers: every case below is refused before a launch
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) & ~15
    p = C.c_void_p(base)
    odd = C.c_void_p(base + 4)
    off = (C.c_int32 * 17)(*range(0, 17 * 8, 8))

    def grid(**kw):
        g = abi.GridT(embeddings=p, offsets=C.cast(off, C.c_void_p), D=2, L=16, H=16, S=1.0, gridtype=1, dtype=abi.RN_F32)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def weights(ind=8, **null):
        w = abi.TorsoWeightsT(def_w0=p, def_w1=p, def_w2=p, tor_w0=p, tor_w1=p, tor_w2=p, ind_dim=ind)
        for k in null:
            setattr(w, k, None)
        return w

    def grads(**null):
        g = abi.TorsoGradsT(def_w0=p, def_w1=p, def_w2=p, tor_w0=p, tor_w1=p, tor_w2=p, ind_code=p)
        for k in null:
            setattr(g, k, None)
        return g
    W = ("def_w0", "def_w1", "def_w2", "tor_w0", "tor_w1", "tor_w2")

    # ---- pack
    def pack(w=weights(), **null):
        a = dict(poses6=p, ind_code=p, image=p)
        a.update({k: None for k in null})
        return lib.rn_train_torso_pack(C.byref(w) if w is not None else None, a["poses6"], a["ind_code"], a["image"], None)
    assert pack(w=None) == RN_ERR_INVALID_ARG and "null weight pointer" in err()
    for name in W:
        assert pack(w=weights(**{name: 1})) == RN_ERR_INVALID_ARG and "null weight pointer" in err(), name
    for name in ("poses6", "ind_code", "image"):
        assert pack(**{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    assert lib.rn_train_torso_pack(C.byref(weights()), p, p, odd, None) == RN_ERR_INVALID_ARG and "16-byte aligned" in err()

    # ---- forward
    def fwd(P=64, g=grid(), shrink=0.8, **null):
        a = dict(xy=p, image=p, alpha=p, color=p, dx=p, wn=p, workspace=p)
        a.update({k: None for k in null})
        return lib.rn_train_torso_forward(a["xy"], P, None, shrink, C.byref(g) if g is not None else None, a["image"], a["alpha"],
                                          a["color"], a["dx"], a["wn"], a["workspace"], None)
    assert fwd(P=0, g=None, xy=1, alpha=1) == 0                                   # nothing to do
    for name in ("xy", "image", "alpha", "color", "dx", "wn", "workspace"):
        assert fwd(**{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    assert fwd(g=None) == RN_ERR_INVALID_ARG and "grid is null" in err()
    assert fwd(g=grid(embeddings=None)) == RN_ERR_INVALID_ARG and "grid is null" in err()
    assert fwd(g=grid(offsets=None)) == RN_ERR_INVALID_ARG and "grid is null" in err()
    for bad in (dict(D=3), dict(L=8), dict(dtype=abi.RN_F16)):
        assert fwd(g=grid(**bad)) == RN_ERR_INVALID_ARG, bad
        assert "D=2" in err() and "L=16" in err() and "fp32" in err() and "C=2" in err(), (bad, err())
    assert fwd(g=grid(embeddings=odd)) == RN_ERR_INVALID_ARG and "8-byte aligned" in err()      # table rows are read as float2
    for bad in (0.0, -1.0):
        assert fwd(shrink=bad) == RN_ERR_INVALID_ARG and "torso_shrink" in err()

    # ---- backward: the upstream gradients may each be null
    def bwd(P=64, g_feat=p, **null):
        a = dict(alpha=p, color=p, image=p, workspace=p)
        a.update({k: None for k in null})
        return lib.rn_train_torso_backward(None, None, None, a["alpha"], a["color"], P, None, a["image"], a["workspace"], g_feat, None)
    assert bwd(P=0, alpha=1, g_feat=None) == 0
    for name in ("alpha", "color", "image", "workspace"):
        assert bwd(**{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    assert bwd(g_feat=None) == RN_ERR_INVALID_ARG and "null pointer" in err()
    assert bwd(g_feat=odd) == RN_ERR_INVALID_ARG and "8-byte aligned" in err()                  # written as float2

    # ---- weight gradients
    def wg(P=64, w=weights(), g=grads(), shrink=0.8, **null):
        a = dict(xy=p, ind_code=p, image=p, workspace=p, wgrad_workspace=p)
        a.update({k: None for k in null})
        return lib.rn_train_torso_weight_grads(C.byref(w) if w is not None else None, a["xy"], shrink, a["ind_code"], P, None, a["image"],
                                               a["workspace"], C.byref(g) if g is not None else None, a["wgrad_workspace"], None)
    assert wg(P=0, w=None, g=None, xy=1) == 0
    assert wg(w=None) == RN_ERR_INVALID_ARG and "null weight pointer" in err()
    for name in W:
        assert wg(w=weights(**{name: 1})) == RN_ERR_INVALID_ARG and "null weight pointer" in err(), name
        assert wg(g=grads(**{name: 1})) == RN_ERR_INVALID_ARG and "null gradient pointer" in err(), name
    for name in ("xy", "image", "workspace", "wgrad_workspace", "ind_code"):
        assert wg(**{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    assert wg(g=None) == RN_ERR_INVALID_ARG and "null pointer" in err()
    assert wg(g=grads(ind_code=1)) == RN_ERR_INVALID_ARG and "null pointer" in err()            # ind_dim = 8 needs its gradient
    assert wg(shrink=0.0) == RN_ERR_INVALID_ARG and "torso_shrink" in err()
