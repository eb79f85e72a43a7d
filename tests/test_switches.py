"""radnerf/switches.py is the one reader of the RN_* switches of the Python side: its table against the environment, the product's
sources and the "Switches" section of INTEGRATION.md.  The module imports nothing but `os`, so it is loaded here by path: no
GPU, no library."""
import glob
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "rad-nerf_amd")


def _load():
    spec = importlib.util.spec_from_file_location("rn_switches", os.path.join(PKG, "radnerf", "switches.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


switches = _load()


def _sources():
    for path in sorted(glob.glob(os.path.join(PKG, "**", "*.py"), recursive=True)):
        with open(path) as f:
            yield os.path.relpath(path, PKG), f.read()


@pytest.fixture
def clean(monkeypatch):
    for name in [n for n in os.environ if n.startswith("RN_")]:
        monkeypatch.delenv(name)


def test_module_imports_only_os():
    with open(os.path.join(PKG, "radnerf", "switches.py")) as f:
        imports = re.findall(r"^\s*(?:import|from)\s+(\S+)", f.read(), flags=re.M)
    assert imports == ["os"]


def test_table_rows_are_well_formed():
    names = [row[0] for row in switches.TABLE]
    assert len(set(names)) == len(names)
    for name, default, accepted, doc in switches.TABLE:
        assert re.fullmatch(r"RN_[A-Z0-9_]+", name)
        assert isinstance(accepted, tuple) and default in accepted and len(set(accepted)) == len(accepted) >= 2
        assert doc and "\n" not in doc


def test_clean_environment_gives_the_defaults(clean):
    for name, default, accepted, _ in switches.TABLE:
        assert switches.get(name) == default
        if set(accepted) == {"0", "1"}:
            assert switches.on(name) == (default == "1")


def test_get_follows_the_environment_after_import(clean, monkeypatch):
    for name, default, accepted, _ in switches.TABLE:
        for value in accepted:
            monkeypatch.setenv(name, value)
            assert switches.get(name) == value
            if set(accepted) == {"0", "1"}:
                assert switches.on(name) == (value == "1")
        monkeypatch.delenv(name)
        assert switches.get(name) == default


@pytest.mark.parametrize("name,value", [("RN_TRAIN_OVERLAP", "true"), ("RN_TRAIN_GLUE", "Torch"), ("RN_TRAIN_HEAD", ""), ("RN_SCATTER", "lbc ")])
def test_a_value_outside_the_accepted_ones_is_an_error(clean, monkeypatch, name, value):
    monkeypatch.setenv(name, value)
    with pytest.raises(ValueError) as err:
        switches.get(name)
    accepted = dict((row[0], row[2]) for row in switches.TABLE)[name]
    assert name in str(err.value) and all(v in str(err.value) for v in accepted)
    if set(accepted) == {"0", "1"}:
        with pytest.raises(ValueError, match=name):
            switches.on(name)


def test_an_unknown_switch_is_an_error(clean):
    with pytest.raises(KeyError):
        switches.get("RN_NO_SUCH_SWITCH")


def test_only_the_table_module_reads_the_environment_for_a_switch():
    reads = re.compile(r"\b(?:environ|getenv)\b.*\bRN_[A-Z0-9_]+|\bRN_[A-Z0-9_]+.*\b(?:environ|getenv)\b")
    found = {rel: [line.strip() for line in text.splitlines() if reads.search(line)] for rel, text in _sources()}
    found = {rel: lines for rel, lines in found.items() if lines and rel != os.path.join("radnerf", "switches.py")}
    assert not found, found
    # and whoever touches the environment at all is known: the table, and the compiler path of the build script
    users = sorted(rel for rel, text in _sources() if re.search(r"\b(?:environ|getenv)\b", text))
    assert users == ["build.py", os.path.join("radnerf", "switches.py")], users


def test_the_table_and_the_product_name_the_same_switches():
    call = re.compile(r"\bswitches\.(get|on)\(\s*([^)]*?)\s*\)")
    read = {}
    for rel, text in _sources():
        for kind, arg in call.findall(text):
            assert re.fullmatch(r"\"RN_[A-Z0-9_]+\"", arg), f"{rel}: switches.{kind}({arg}): the name is not a literal"
            read.setdefault(arg.strip('"'), set()).add(kind)
    accepted = {row[0]: row[2] for row in switches.TABLE}
    assert set(read) == set(accepted), (sorted(set(read) - set(accepted)), sorted(set(accepted) - set(read)))
    for name, kinds in read.items():
        if "on" in kinds:
            assert set(accepted[name]) == {"0", "1"}, name


def test_integration_md_holds_the_generated_table():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = re.search(r"^## Switches\n(.*?)(?=^## |\Z)", text, flags=re.M | re.S)
    assert section, "INTEGRATION.md has no '## Switches' section"
    assert section.group(1).strip() == switches.markdown().strip()
