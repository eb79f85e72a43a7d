"""rn_torso_select and rn_train_torso_loss (the two kernels of a device-resident torso step, include/radnerf_train.h): declared,
exported, in the ctypes table in header order, and refusing bad arguments before anything touches a GPU.  Modelled on
tests/test_train_torso_abi.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RN_ERR_INVALID_ARG = -1
ENTRIES = [("rn_torso_select", "int", 10), ("rn_train_torso_loss", "int", 16)]


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
        assert restype is C.c_int, name
    assert at == sorted(at) and [i for _, i in at] == sorted(i for _, i in at)        # header order = table order
    assert all(i > names.index("rn_train_torso_weight_grads") for _, i in at)       # after what the header had before


def test_entries_refuse_bad_arguments(hiplib):
    """Null required pointers, G < 2, a misaligned xy_c and row strides that cannot hold a pixel come back as RN_ERR_INVALID_ARG
    with a message; the loss with N == 0 is a no-op, with P == 0 it needs none of the compact buffers' checks to pass first."""
    lib, err = hiplib._lib, hiplib.last_error
    with open(os.path.join(ROOT, "include", "radnerf_hip.h")) as f:
        assert int(re.search(r"#define\s+RN_ERR_INVALID_ARG\s+\((-?\d+)\)", f.read()).group(1)) == RN_ERR_INVALID_ARG
    # host memory stands in for the device buffers: every case below is refused before a launch
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) & ~15
    p = C.c_void_p(base)
    odd = C.c_void_p(base + 4)

    # ---- select
    def select(N=64, G=128, xy_c=p, **null):
        a = dict(bg_coords=p, grid=p, covered=p, count=p)
        a.update({k: None for k in null})
        return lib.rn_torso_select(a["bg_coords"], N, a["grid"], G, 0.5, None, a["covered"], xy_c, a["count"], None)
    for name in ("bg_coords", "grid", "covered", "count"):
        assert select(**{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    assert select(xy_c=None) == RN_ERR_INVALID_ARG and "null pointer" in err()
    assert select(N=0, count=1) == RN_ERR_INVALID_ARG and "null pointer" in err()      # N == 0 still has a count to write
    for G in (0, 1):
        assert select(G=G) == RN_ERR_INVALID_ARG and "grid_size" in err(), G
    assert select(xy_c=odd) == RN_ERR_INVALID_ARG and "8-byte aligned" in err()             # written as float2
    assert select(N=(1 << 30) + 1) == RN_ERR_INVALID_ARG and "2^30" in err()                # indices are int32

    # ---- loss
    def loss(N=64, P=32, bg_stride=3, target_stride=3, **null):
        a = dict(alpha_c=p, color_c=p, covered=p, bg=p, target=p, loss=p, pred=p, alpha_full=p, g_alpha=p, g_color=p)
        a.update({k: None for k in null})
        return lib.rn_train_torso_loss(a["alpha_c"], a["color_c"], a["covered"], P, None, a["bg"], bg_stride, a["target"], target_stride,
                                       N, a["loss"], a["pred"], a["alpha_full"], a["g_alpha"], a["g_color"], None)
    assert loss(N=0, bg=1, loss=1, alpha_c=1) == 0                                    # nothing to do
    for name in ("alpha_c", "color_c", "covered", "bg", "target", "loss", "pred", "alpha_full", "g_alpha", "g_color"):
        assert loss(**{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    for name in ("bg", "target", "loss", "pred", "alpha_full"):                        # P == 0: these are still required
        assert loss(P=0, **{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    for bad in (dict(bg_stride=0), dict(target_stride=0), dict(bg_stride=2), dict(target_stride=1)):
        assert loss(**bad) == RN_ERR_INVALID_ARG and "stride" in err(), bad
