"""The camera-pose entry points (rn_camera_rays_forward / _workspace / _backward, include/radnerf_train.h) are declared, exported and
mirrored in radnerf_hip/abi.py, refuse bad arguments before anything touches a GPU -- and the pose arithmetic they share
(csrc/rn_camera_dev.h: angles -> R, G -> grad_a) is right: built into a stand-alone host program and compared with float64 torch
autograd through rays.euler_angles_to_matrix.  No GPU anywhere in this file."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import torch

from test_abi import SCALARS, _header_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rad-nerf_amd", "csrc")
RN_ERR_INVALID_ARG = -1

# name -> (return type, [(base type, is pointer), ...]) as the issue's signatures read
EXPECTED = {
    "rn_camera_rays_forward": ("int", [("float", True)] * 4 + [("int64_t", True), ("uint32_t", False), ("uint32_t", False),
                                                               ("float", True), ("float", True), ("rn_stream_t", False)]),
    "rn_camera_rays_workspace": ("size_t", [("uint32_t", False)]),
    "rn_camera_rays_backward": ("int", [("float", True)] * 4 + [("int64_t", True), ("uint32_t", False), ("uint32_t", False),
                                                                ("float", True), ("float", True), ("void", True), ("rn_stream_t", False)]),
}

PROGRAM = r"""
#include <stdio.h>
#include "rn_camera_dev.h"
// stdin: one case per line, 3 angles in degrees and the 9 entries of G (row-major); stdout: 9 entries of R, 3 of grad_a
int main() {
    float deg[3];
    double G[9];
    for (;;) {
        if (scanf("%f %f %f", &deg[0], &deg[1], &deg[2]) != 3) break;
        for (int e = 0; e < 9; e++)
            if (scanf("%lf", &G[e]) != 1) return 2;
        float a[3], R[9], ga[3];
        rn::cam::pose_angles(deg, a);
        rn::cam::pose_matrix(a, R);
        rn::cam::pose_angle_grads(G, a, ga);
        for (int e = 0; e < 9; e++) printf("%.9g ", R[e]);
        printf("%.9g %.9g %.9g\n", ga[0], ga[1], ga[2]);
    }
    return 0;
}
"""


def test_entry_points_are_declared_exported_and_in_the_table(hiplib):
    from radnerf_hip import abi
    decls = _header_functions()
    names = list(abi.FUNCTIONS)
    for name, (ret, params) in EXPECTED.items():
        assert name in decls, f"{name} is not declared in include/radnerf_train.h"
        assert decls[name] == (ret, params), (name, decls[name])
        assert name in abi.FUNCTIONS, f"{name} is missing from radnerf_hip/abi.py"
        restype, argtypes = abi.FUNCTIONS[name]
        assert restype is (C.c_size_t if ret == "size_t" else C.c_int) and len(argtypes) == len(params), name
        for (base, is_ptr), ctype in zip(params, argtypes):
            assert ctype is (C.c_void_p if (is_ptr or base == "rn_stream_t") else SCALARS[base]), (name, base, ctype)
        fn = getattr(hiplib._lib, name)                   # AttributeError: the library does not export it
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert names.index("rn_camera_rays_forward") < names.index("rn_camera_rays_workspace") < names.index("rn_camera_rays_backward")


def test_entry_points_refuse_bad_arguments(hiplib):
    """Null pointers and tables without rows come back as RN_ERR_INVALID_ARG with a message; a forward over no rays is a no-op;
    the workspace is 12 floats per 256 rays."""
    lib, err = hiplib._lib, hiplib.last_error
    buf = (C.c_float * 64)()
    idx = (C.c_int64 * 1)(0)
    p, ip = C.cast(buf, C.c_void_p), C.cast(idx, C.c_void_p)
    fwd, bwd, ws = lib.rn_camera_rays_forward, lib.rn_camera_rays_backward, lib.rn_camera_rays_workspace
    assert fwd(None, None, None, None, None, 0, 0, None, None, None) == 0                     # nothing to do
    for k in range(9):
        if k in (5, 6):
            continue
        args = [p, p, p, p, ip, 8, 4, p, p]
        args[k] = None
        assert fwd(*args, None) == RN_ERR_INVALID_ARG and "null pointer" in err(), k
    assert fwd(p, p, p, p, ip, 0, 4, p, p, None) == RN_ERR_INVALID_ARG and "no rows" in err()
    for k in (0, 1, 2, 3, 4, 7, 8, 9):
        args = [p, p, p, p, ip, 8, 4, p, p, p]
        args[k] = None
        assert bwd(*args, None) == RN_ERR_INVALID_ARG and "null pointer" in err(), k
    assert bwd(p, p, p, p, ip, 0, 4, p, p, p, None) == RN_ERR_INVALID_ARG and "no rows" in err()
    assert [int(ws(n)) for n in (0, 1, 256, 257, 4096)] == [48, 48, 48, 96, 16 * 48]


def test_pose_math_against_float64_autograd(tmp_path):
    """R and grad_a of csrc/rn_camera_dev.h, compiled for the host (RN_POSE_CXXFLAGS adds flags, e.g. a sanitizer's), for twelve
    seeded angle triples in +-10 degrees (the first all zero) and seeded G matrices, against float64 autograd through
    rays.euler_angles_to_matrix on the same fp32 inputs.  Bar: max-normalised error <= 1e-6 -- fp32 eps is 6e-8, R's entries and
    the derivative sums have fewer than ten terms of magnitude <= 1."""
    from radnerf.rays import euler_angles_to_matrix
    cxx = shutil.which("g++") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "pose.cpp", tmp_path / "pose"
    src.write_text(PROGRAM)
    flags = os.environ.get("RN_POSE_CXXFLAGS", "").split()
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC] + flags + ["-o", str(exe), str(src), "-lm"], check=True)
    rng = np.random.default_rng(20)
    deg = rng.uniform(-10, 10, (12, 3)).astype(np.float32)
    deg[0] = 0
    G = rng.uniform(-1, 1, (12, 9)).astype(np.float32)
    G[1] = 0
    text = "".join(" ".join(f"{float(v):.9g}" for v in list(d) + list(g)) + "\n" for d, g in zip(deg, G))
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.array([[float(v) for v in line.split()] for line in r.stdout.strip().split("\n")])
    assert got.shape == (12, 12)
    a = (torch.from_numpy(deg).double() / 180 * np.pi + 1e-8).requires_grad_(True)
    R = euler_angles_to_matrix(a)                                                           # [12, 3, 3]
    (R * torch.from_numpy(G).double().view(12, 3, 3)).sum().backward()
    R64, ga64 = R.detach().numpy().reshape(12, 9), a.grad.numpy()
    e_R = float(np.abs(got[:, :9] - R64).max() / np.abs(R64).max())
    e_g = float(np.abs(got[:, 9:] - ga64).max() / np.abs(ga64).max())
    print(f"pose math on the host: R {e_R:.3e}  grad_a {e_g:.3e}")
    assert np.all(got[1, 9:] == 0.0)                                                        # G = 0: no gradient
    assert e_R <= 1e-6 and e_g <= 1e-6, (e_R, e_g)
