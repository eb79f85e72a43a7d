#!/usr/bin/env python3
"""Compare the gfx950 code objects of two trees, kernel by kernel (no GPU needed).

    python tools/isa_diff.py <tree A> <tree B> [--only rn_mlp.hip,rn_train_head.hip] [--all]

Every rad-nerf_amd/csrc/*.hip of both trees is compiled with build.py's CXXFLAGS plus --save-temps into a scratch directory;
`llvm-objdump -d --no-show-raw-insn --no-leading-addr` of each gfx950 object is cut per kernel symbol and the instruction text
compared.  Per kernel: identical / differs / only in one tree, and VGPR / AGPR / SGPR / LDS bytes / scratch bytes of both
sides from the metadata of the .s file.  Identical kernels are counted per file and listed only with --all.
"""
import argparse
import importlib.util
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

LLVM = "/opt/rocm/llvm/bin"
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def load_build(tree):
    spec = importlib.util.spec_from_file_location("rn_build", os.path.join(tree, "rad-nerf_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_one(build, src, out):
    """-> {kernel name: (instruction text, resource figures)} of one source file"""
    os.makedirs(out, exist_ok=True)
    cmd = [build.HIPCC] + build.CXXFLAGS + ["--save-temps", "-c", os.path.join(build.CSRC, src), "-o", os.path.join(out, "host.o")]
    subprocess.run(cmd, cwd=out, check=True, capture_output=True)
    stem = os.path.join(out, f"{src[:-4]}-hip-amdgcn-amd-amdhsa-{build.ARCH}")
    res, cur = {}, None
    for line in open(stem + ".s"):                      # kernel entries of .amdgpu_metadata: keys at a fixed indentation
        m = re.match(r"^(  - |    )\.(\w+):\s*(.*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is not None:
            cur[m.group(2)] = m.group(3).strip()
            if m.group(2) == "name":
                res[cur["name"]] = cur
    dump = [os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", stem + ".o"]
    text = subprocess.run(dump, check=True, capture_output=True, text=True).stdout
    label = re.compile(r"^[0-9a-f]*\s*<(.+)>:$")
    demangled = [m.group(1) for m in map(label.match, subprocess.run(dump + ["-C"], check=True, capture_output=True,
                                                                     text=True).stdout.splitlines()) if m]
    kernels, pretty, sym = {}, {}, None
    for line in text.splitlines():
        m = label.match(line)
        if m:
            sym = m.group(1)
            pretty[sym] = demangled[len(pretty)]        # the labels come in the same order with and without -C
            continue
        if sym in res and line.strip():
            kernels.setdefault(sym, []).append(line.split("//")[0].rstrip())
    return {pretty[k].split("(")[0]: ("\n".join(v), tuple(int(res[k].get(key, 0)) for key in KEYS)) for k, v in kernels.items()}


def compile_tree(tree, out, only):
    build = load_build(tree)
    srcs = [s for s in build._sources() if not only or s in only]
    with ThreadPoolExecutor(max_workers=4) as ex:
        return dict(zip(srcs, ex.map(lambda s: compile_one(build, s, os.path.join(out, s[:-4])), srcs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--only", default="", help="comma-separated source files (default: all)")
    ap.add_argument("--all", action="store_true", help="list identical kernels too")
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    with tempfile.TemporaryDirectory(prefix="isa_diff_") as tmp:
        A = compile_tree(os.path.abspath(a.tree_a), os.path.join(tmp, "a"), only)
        B = compile_tree(os.path.abspath(a.tree_b), os.path.join(tmp, "b"), only)
    fig = lambda r: "vgpr %3d agpr %3d sgpr %3d lds %6d scratch %d" % r
    differs = 0
    for src in sorted(set(A) | set(B)):
        ka, kb = A.get(src, {}), B.get(src, {})
        same = [k for k in ka if k in kb and ka[k][0] == kb[k][0]]
        print(f"{src}: {len(same)} of {len(set(ka) | set(kb))} kernels identical")
        for k in sorted(set(ka) | set(kb)):
            state = "identical" if k in same else ("differs" if k in ka and k in kb else ("only in A" if k in ka else "only in B"))
            if state == "identical" and not a.all:
                continue
            differs += state != "identical"
            print(f"  {state:9s} {k}")
            for side, t in (("A", ka), ("B", kb)):
                if k in t and state != "identical":
                    print(f"            {side}: {fig(t[k][1])}  ({t[k][0].count(chr(10)) + 1} instructions)")
    return 1 if differs else 0


if __name__ == "__main__":
    sys.exit(main())
