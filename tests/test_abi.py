"""The C-ABI library loads on a CPU-only box, and radnerf_hip.abi -- the one Python mirror of include/*.h -- agrees with
the headers in full: the set of functions, every parameter and return type, every struct's layout, every constant."""
import ctypes
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
HEADERS = ("radnerf_hip.h", "radnerf_fused.h", "radnerf_train.h")

SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t,
           "uint8_t": ctypes.c_uint8, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64}
RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "uint32_t": ctypes.c_uint32, "const char *": ctypes.c_char_p}


def _header_text(fn):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, fn)).read(), flags=re.S)


def _c_type(words):
    """'const float *' -> ('float', True); 'uint32_t' -> ('uint32_t', False)."""
    base = [w for w in words.replace("*", " ").split() if w != "const"]
    assert len(base) == 1, words
    return base[0], "*" in words


def _header_functions():
    """{name: (return type, [(base type, is pointer), ...])} of every function the headers declare, in header order."""
    decls = {}
    for fn in HEADERS:
        for m in re.finditer(r"^((?:const\s+)?\w+\s*\*?)\s*\b(rn_\w+)\s*\(([^;{()]*)\)\s*;", _header_text(fn), flags=re.M):
            ret, name, args = " ".join(m.group(1).split()), m.group(2), m.group(3).strip()
            assert name not in decls, name
            params = []
            for a in ([] if args in ("", "void") else args.split(",")):
                words, pname = re.fullmatch(r"\s*(.*?)(\w+)\s*", a, flags=re.S).groups()
                params.append(_c_type(words))
            decls[name] = (ret, params)
    return decls


def _header_structs():
    """{rn_X_t: [(field, base type, is pointer, array length or 0), ...]} in declaration order.  Declarators come as
    `const float *a, *b;`, `uint32_t D, L, H;` and `const float *conv_w[4], *conv_b[4];`."""
    structs = {}
    for fn in HEADERS:
        for m in re.finditer(r"typedef\s+struct\s*\{(.*?)\}\s*(rn_\w+_t)\s*;", _header_text(fn), flags=re.S):
            fields = []
            for decl in filter(None, (d.strip() for d in m.group(1).split(";"))):
                base, rest = re.fullmatch(r"((?:const\s+)?\w+)\s*(.*)", decl, flags=re.S).groups()
                for d in rest.split(","):
                    star, name, n = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*", d).groups()
                    fields.append((name, _c_type(base)[0], bool(star), int(n or 0)))
            structs[m.group(2)] = fields
    return structs


def _header_constants():
    out = {}
    for fn in HEADERS:
        for m in re.finditer(r"^#define\s+(RN_\w+)\s+\(?(-?\d+)u?\)?\s*$", _header_text(fn), flags=re.M):
            out[m.group(1)] = int(m.group(2))
    return out


def _mirrors(abi):
    """{rn_X_t: the ctypes.Structure of radnerf_hip.abi that mirrors it}."""
    out = {}
    for v in vars(abi).values():
        if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure:
            assert v.c_name not in out, v.c_name
            out[v.c_name] = v
    return out


def _pointer_ok(ctype, base, mirrors):
    """A C pointer to `base` may be bound as void * or as a ctypes pointer to the matching type; a pointer to a struct of
    the ABI must be the typed pointer to its mirror."""
    if base in mirrors:
        return ctype is ctypes.POINTER(mirrors[base])
    if ctype is ctypes.c_void_p:
        return True
    return base in SCALARS and ctype is ctypes.POINTER(SCALARS[base])


def test_parser_sees_the_whole_boundary():
    """The checks below are only as good as the parser: pin what it finds in today's headers (update when one grows)."""
    fns, structs, consts = _header_functions(), _header_structs(), _header_constants()
    per_header = [len(re.findall(r"^(?:const\s+)?\w+\s*\*?\s*\brn_\w+\s*\(", _header_text(h), flags=re.M)) for h in HEADERS]
    assert sum(per_header) == len(fns) and len(fns) >= 105
    assert len(structs) >= 9 and sum(len(f) for f in structs.values()) >= 96
    assert sum(1 for r, ps in fns.values() for p in ps if p == ("double", False)) >= 4
    assert {r for r, _ in fns.values()} == set(RETURNS)
    assert consts["RN_ERR_INVALID_ARG"] == -1 and consts["RN_LOOP_COOP"] == 4 and consts["RN_HEAD_ST_STALLED"] == 22
    assert structs["rn_grid_t"][2:5] == [("D", "uint32_t", False, 0), ("L", "uint32_t", False, 0), ("H", "uint32_t", False, 0)]
    assert structs["rn_audio_weights_t"][1] == ("conv_b", "float", True, 4)
    assert structs["rn_nerf_weights_t"][1] == ("amb_w1", "float", True, 0)


def test_library_loads_and_exports_every_declared_symbol(hiplib):
    decls = _header_functions()
    assert len(decls) >= 25
    lib = ctypes.CDLL(hiplib.LIB_PATH)
    for name in decls:
        assert hasattr(lib, name), f"{name} declared in include/ but not exported"
    assert set(hiplib.exported_symbols()) == set(decls)


def test_table_has_exactly_the_declared_functions(hiplib):
    from radnerf_hip import abi
    decls = _header_functions()
    assert list(abi.FUNCTIONS) == list(decls), (set(decls) ^ set(abi.FUNCTIONS))     # same set, in header order
    for name in abi.FUNCTIONS:                       # ... and bind() put every entry on the loaded library
        fn = getattr(hiplib._lib, name)
        assert (fn.restype, list(fn.argtypes)) == (abi.FUNCTIONS[name][0], list(abi.FUNCTIONS[name][1])), name


def test_every_parameter_and_return_type_matches_the_header(hiplib):
    from radnerf_hip import abi
    mirrors = _mirrors(abi)
    for name, (ret, params) in _header_functions().items():
        restype, argtypes = abi.FUNCTIONS[name]
        assert restype is RETURNS[ret], f"{name}: returns {ret}, bound as {restype}"
        assert len(argtypes) == len(params), f"{name}: header has {len(params)} args, binding has {len(argtypes)}"
        for i, ((base, is_ptr), ctype) in enumerate(zip(params, argtypes)):
            if base == "rn_stream_t":
                ok = ctype is ctypes.c_void_p and not is_ptr
            elif is_ptr:
                ok = _pointer_ok(ctype, base, mirrors)
            else:
                ok = ctype is SCALARS[base]
            assert ok, f"{name}: argument {i} is {base}{' *' if is_ptr else ''}, bound as {ctype}"


def test_struct_mirrors_have_the_compilers_layout(hiplib, tmp_path):
    from radnerf_hip import abi
    structs, mirrors = _header_structs(), _mirrors(abi)
    assert set(mirrors) == set(structs)
    lines = ["#include <stdio.h>", "#include <stddef.h>"] + [f'#include "{h}"' for h in HEADERS] + ["int main(void) {"]
    for sname, fields in structs.items():
        lines.append(f'    printf("{sname} %zu\\n", sizeof({sname}));')
        for fname, *_ in fields:
            lines.append(f'    printf("{sname}.{fname} %zu %zu\\n", offsetof({sname}, {fname}), sizeof((({sname} *)0)->{fname}));')
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([shutil.which("gcc") or "cc", "-std=c99", "-I", INCLUDE, "-o", str(exe), str(src)], check=True)
    said = {}
    for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split("\n"):
        if line:
            key, *nums = line.split()
            said[key] = tuple(int(n) for n in nums)
    for sname, fields in structs.items():
        cls = mirrors[sname]
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields], sname
        assert ctypes.sizeof(cls) == said[sname][0], sname
        for (fname, ctype), (_, base, is_ptr, n) in zip(cls._fields_, fields):
            desc = getattr(cls, fname)
            assert (desc.offset, desc.size) == said[f"{sname}.{fname}"], f"{sname}.{fname}"
            elem = ctype._type_ if n else ctype
            assert not n or (issubclass(ctype, ctypes.Array) and ctype._length_ == n), f"{sname}.{fname}"
            assert _pointer_ok(elem, base, mirrors) if is_ptr else elem is SCALARS[base], f"{sname}.{fname}: {base} bound as {elem}"


def test_constants_equal_the_headers_defines(hiplib):
    from radnerf_hip import abi
    defines = _header_constants()
    mine = {k: v for k, v in vars(abi).items() if re.fullmatch(r"RN_[A-Z0-9_]+", k)}
    assert len(mine) >= 15
    for name, value in mine.items():
        assert name in defines, f"abi.{name} has no #define in include/"
        assert value == defines[name], f"abi.{name} = {value}, header says {defines[name]}"
    for name in ("RN_F32", "RN_F16", "RN_LAYOUT_LBC", "RN_LAYOUT_BLC", "RN_LAYOUT_BLC_LEVELMAJOR"):
        assert getattr(hiplib, name) == defines[name]


def test_bindings_live_in_one_place():
    """Signatures, return types and struct mirrors are declared in radnerf_hip/abi.py and nowhere else in the package."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rad-nerf_amd")):
        for f in files:
            path = os.path.join(dirpath, f)
            if f.endswith(".py") and os.path.relpath(path, ROOT) != os.path.join("rad-nerf_amd", "radnerf_hip", "abi.py"):
                if re.search(r"\bargtypes\b|\brestype\b|\bStructure\b", open(path).read()):
                    bad.append(path)
    assert not bad, bad


def test_version_and_error_channel(hiplib):
    assert hiplib.version() >= 100
    assert isinstance(hiplib.last_error(), str)
    # bad arguments are rejected on the host before anything touches a device
    rc = hiplib._lib.rn_sh_encode_forward(1, 1, 4, 2, 4, None, None)
    assert rc == -1 and "input dim == 3" in hiplib.last_error()
    rc = hiplib._lib.rn_grid_encode_forward(1, 1, 1, 1, 4, 3, 3, 16, 0.5, 16, None, 0, 0, 0, 0, 0, None)
    assert rc == -1 and "C must be 1, 2, 4, or 8" in hiplib.last_error()
    rc = hiplib._lib.rn_grid_encode_forward(1, 1, 1, 1, 4, 7, 2, 16, 0.5, 16, None, 0, 0, 0, 0, 0, None)
    assert rc == -1 and "D must be" in hiplib.last_error()


def test_no_oracle_or_cpu_fallback_in_product_tree():
    """The product package must never import, load or link anything under oracle/."""
    bad = []
    for dirpath, _, files in os.walk(os.path.join(ROOT, "rad-nerf_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                if re.search(r"pyoracle|radnerf_oracle|libradnerf_oracle|orc_\w+\(", text):
                    bad.append(os.path.join(dirpath, f))
    assert not bad, bad


def test_round2_entry_points_refuse_bad_arguments(hiplib):
    """The argument checks of the training-side entry points run before anything touches a GPU: unsupported shapes and null
    pointers come back as RN_ERR_INVALID_ARG with a message (no launch, no CPU fallback)."""
    lib, err = hiplib._lib, hiplib.last_error
    assert lib.rn_mlp64_image_floats(96, 2, 3) > 0 and lib.rn_mlp64_image_floats(65, 65, 3) > 0 and lib.rn_mlp64_image_floats(84, 3, 2) > 0
    assert lib.rn_mlp64_image_floats(128, 2, 3) == 0 and lib.rn_mlp64_image_floats(65, 7, 3) == 0 and lib.rn_mlp64_image_floats(65, 65, 4) == 0
    assert lib.rn_mlp64_pack(None, 128, None, None, 128, 2, 3, None, None) != 0 and "unsupported shape" in err()
    assert lib.rn_mlp64_pack(None, 32, None, None, 64, 2, 3, None, None) != 0 and "ld0" in err()
    assert lib.rn_mlp64_forward(None, 0, None, None, 65, 65, 3, None, None, None, None) == 0        # M = 0: nothing to do
    assert lib.rn_mlp64_forward(None, 64, None, None, 65, 65, 3, None, None, None, None) != 0 and "null pointer" in err()
    assert lib.rn_adam_step(None, 0, 0.9, 0.99, 1e-15, None, None, None) != 0 and "step counter" in err()
    assert lib.rn_train_loss(None, None, None, None, None, None, 0, None, None, None, None, None) != 0 and "N must be positive" in err()
    assert lib.rn_head_mid_forward(None, None, 10, 16, None, None, None) != 0 and "null pointer" in err()
    assert lib.rn_audio_encode_windows_backward(None, None, 1, None, None, None, None, None) != 0 and "null weights" in err()
    assert lib.rn_march_rays_train_budget(None, None, None, 1.0, 0.0, 16, 64, 1, 128, 1000, *([None] * 11)) != 0 and "null pointer" in err()
