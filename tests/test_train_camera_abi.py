"""rn_train_head_input_grads (the position / direction gradients of the fused training head, include/radnerf_train.h): declared,
exported, in the ctypes table, and refusing bad arguments before anything touches a GPU.  Modelled on
tests/test_abi.py::test_round2_entry_points_refuse_bad_arguments."""
import ctypes as C
import os
import re

NAME = "rn_train_head_input_grads"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RN_ERR_INVALID_ARG = -1


def test_input_grads_is_declared_exported_and_in_the_table(hiplib):
    from radnerf_hip import abi
    header = open(os.path.join(ROOT, "include", "radnerf_train.h")).read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header), "not declared in include/radnerf_train.h"
    assert NAME in abi.FUNCTIONS
    names = list(abi.FUNCTIONS)
    assert names.index("rn_train_head_backward") < names.index(NAME) < names.index("rn_train_head_weight_grads")   # header order
    fn = getattr(hiplib._lib, NAME)                       # AttributeError: the library does not export it
    restype, argtypes = abi.FUNCTIONS[NAME]
    assert fn.restype is restype and list(fn.argtypes) == argtypes and len(argtypes) == 12


def test_input_grads_refuses_bad_arguments(hiplib):
    """Null required pointers and a grid the kernel is not built for (D != 3, L != 16, a non-fp32 table) come back as
    RN_ERR_INVALID_ARG with a message; M == 0 is a no-op.  rn_grid_t carries no channel count -- its tables are [rows, 2] by
    type -- so C != 2 cannot be expressed through this ABI; the refusal message names the C = 2 requirement."""
    from radnerf_hip import abi
    lib, err = hiplib._lib, hiplib.last_error
    fn = getattr(lib, NAME)
    with open(os.path.join(ROOT, "include", "radnerf_hip.h")) as f:
        assert int(re.search(r"#define\s+RN_ERR_INVALID_ARG\s+\((-?\d+)\)", f.read()).group(1)) == RN_ERR_INVALID_ARG
    # host memory stands in for the device buffers: every case below is refused before a launch
    buf = (C.c_float * 64)()
    off = (C.c_int32 * 17)(*range(0, 17 * 8, 8))
    p = C.cast(buf, C.c_void_p)

    def grid(**kw):
        g = abi.GridT(embeddings=p, offsets=C.cast(off, C.c_void_p), D=3, L=16, H=16, S=1.0, gridtype=1, dtype=abi.RN_F32)
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    def call(M=64, g=None, **null):
        a = dict(xn=p, dirs=p, grad_enc_x=p, image=p, workspace=p, grad_xyzs=p, grad_dirs=p)
        a.update({k: None for k in null})
        gp = C.byref(g) if g is not None else None
        return fn(a["xn"], a["dirs"], a["grad_enc_x"], M, None, gp, a["image"], a["workspace"], 1.0, a["grad_xyzs"], a["grad_dirs"], None)

    assert call(M=0, g=None, xn=1, grad_xyzs=1) == 0                          # nothing to do
    for name in ("xn", "dirs", "grad_enc_x", "image", "workspace", "grad_xyzs", "grad_dirs"):
        assert call(g=grid(), **{name: 1}) == RN_ERR_INVALID_ARG and "null pointer" in err(), name
    assert call(g=None) == RN_ERR_INVALID_ARG and "grid is null" in err()
    assert call(g=grid(embeddings=None)) == RN_ERR_INVALID_ARG and "grid is null" in err()
    assert call(g=grid(offsets=None)) == RN_ERR_INVALID_ARG and "grid is null" in err()
    for bad in (dict(D=2), dict(D=4), dict(L=8), dict(dtype=abi.RN_F16)):
        assert call(g=grid(**bad)) == RN_ERR_INVALID_ARG, bad
        assert "D=3" in err() and "fp32" in err() and "C=2" in err(), (bad, err())
    odd = C.c_void_p(C.addressof(buf) + 4)                                  # feature gradients are read as float2
    assert fn(p, p, odd, 64, None, C.byref(grid()), p, p, 1.0, p, p, None) == RN_ERR_INVALID_ARG and "8-byte aligned" in err()
    assert fn(p, p, p, 64, None, C.byref(grid()), p, p, 0.0, p, p, None) == RN_ERR_INVALID_ARG and "bound" in err()
