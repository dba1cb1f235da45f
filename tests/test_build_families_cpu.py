"""What every build family states the same way (tests/build_families.py), asserted once over the table: the
names and values of the builds in the Python package, in include/sbx.h and in include/sbx_mainimage.hpp, and the table's own
consistency with the committed fixtures and, where it is present, with the reference's headers."""
import os
import subprocess

import pytest

from tests.app_checks import check_mainimage_selects
from tests.build_families import FAMILIES, fixture_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = [(family, build) for family, fam in FAMILIES.items() for build in fam["builds"]]
LAST = max(b["value"] for fam in FAMILIES.values() for b in fam["builds"].values())
PINNED = 19                                         # shaderbox_amd.APPS keeps the apps below this value; later ones are in MORE_APPS


def _define(app):
    return "APP_" + app.upper()


@pytest.mark.parametrize("family", FAMILIES)
def test_python_names(family):
    import shaderbox_amd
    fam = FAMILIES[family]
    M = __import__("tests.%s_builds_model" % family, fromlist=["APP_OF"])
    for build, b in fam["builds"].items():
        name, value = b["name"], b["value"]
        assert name == _define(b["app"]) and b["app"] == "%s_%s" % (fam["shipped"][0], build)
        assert getattr(shaderbox_amd, name) == value == shaderbox_amd.ALL_APPS[name]
        # APPS is pinned to its entries: a build appended after them is in MORE_APPS alone
        assert (shaderbox_amd.APPS[name] == value and name not in shaderbox_amd.MORE_APPS) if value < PINNED else \
               (shaderbox_amd.MORE_APPS[name] == value and name not in shaderbox_amd.APPS)
        assert shaderbox_amd.app_id(b["app"]) == value == shaderbox_amd.app_id(name)
        assert shaderbox_amd.app_id(getattr(M, "APP_OF", {build: b["app"]})[build]) == value
    for app, value in (fam["shipped"],) + fam.get("also_shipped", ()):
        assert shaderbox_amd.app_id(app) == value == shaderbox_amd.app_id(_define(app)) == shaderbox_amd.APPS[_define(app)]
    # appended: no value renumbered, the table dense
    assert sorted(shaderbox_amd.ALL_APPS.values()) == list(range(len(shaderbox_amd.ALL_APPS))) and len(shaderbox_amd.ALL_APPS) >= LAST + 1
    assert all(shaderbox_amd.ALL_APPS[k] == v for k, v in shaderbox_amd.APPS.items())
    assert sorted(shaderbox_amd.APPS.values()) == list(range(PINNED))          # APPS keeps its pinned entries
    assert shaderbox_amd.SBX_ABI_VERSION == 2


@pytest.mark.parametrize("family", FAMILIES)
def test_enum_lines_of_the_header(family, tmp_path):
    """every enumerator of the family stands in include/sbx.h exactly once, with its value, and the compiler reads the same values:
    the shipped apps', the builds' and that of the enumerator before the first build (appended: nothing renumbered)"""
    import shaderbox_amd
    fam = FAMILIES[family]
    want = {"SBX_" + _define(app): value for app, value in (fam["shipped"],) + fam.get("also_shipped", ())}
    want.update(("SBX_" + b["name"], b["value"]) for b in fam["builds"].values())
    code = [ln.split("/*")[0].strip().rstrip(",") for ln in open(os.path.join(ROOT, "include", "sbx.h")).read().splitlines()]
    for name, value in want.items():
        assert code.count("%s = %d" % (name, value)) == 1, (name, value)
    assert code.count("#define SBX_ABI_VERSION 2") == 1
    first = min(b["value"] for b in fam["builds"].values())
    want.update(("SBX_" + k, v) for k, v in shaderbox_amd.ALL_APPS.items() if v == first - 1)
    src = tmp_path / "enum.cpp"
    src.write_text('#include "sbx.h"\nstatic_assert(%s && SBX_ABI_VERSION == 2, "appended");\n' % " && ".join("%s == %d" % kv for kv in want.items()))
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


def _selections():
    """(defines, the app sbx_mainimage.hpp is to select): a build's define alone, before and after the shipped define; the shipped
    define alone; and the family's other defines of the header"""
    for family, fam in FAMILIES.items():
        shipped = _define(fam["shipped"][0])
        for b in fam["builds"].values():
            for defines in ([b["name"]], [shipped, b["name"]], [b["name"], shipped]):
                yield pytest.param(defines, "SBX_" + b["name"], id="-".join(defines))
        for name in (shipped,) + fam.get("mainimage_also", ()):
            yield pytest.param([name], "SBX_" + name, id=name)


@pytest.mark.parametrize("defines,want", _selections())
def test_mainimage_header_selects_the_build(defines, want):
    check_mainimage_selects(defines, want)


@pytest.mark.parametrize("family,build", BUILDS)
def test_table_is_consistent(family, build):
    """the fixture of every build is there, and decodes with the keys and uniforms the table states; its app is the package's"""
    import shaderbox_amd
    from tests.model_common import builds_fixture
    fam, b = FAMILIES[family], FAMILIES[family]["builds"][build]
    assert os.path.isfile(fixture_path(os.path.join(ROOT, "tests"), family, build))
    assert shaderbox_amd.ALL_APPS[b["name"]] == b["value"] == shaderbox_amd.app_id(b["app"])
    fx = builds_fixture(family, build)
    assert len(fx["frames"]) == len(fam["uniforms"]) + len(fam.get("aux_sets", ()))
    assert len(fx["big_frames"]) == (len(fam["big"]["uniforms"]) if "min_big" in b else 0)
    assert ("points" in fx) == bool(fam["points"])
    at, old, new = b["edit"]
    assert at >= 1 and old and new != old


@pytest.mark.parametrize("family,build", BUILDS)
def test_edit_lines_are_the_reference_headers(family, build):
    from oracle.oracle import reference_root
    path = os.path.join(reference_root(), "src", FAMILIES[family]["header"])
    if not os.path.isfile(path):
        pytest.skip("reference tree not present")
    at, old, _ = FAMILIES[family]["builds"][build]["edit"]
    lines = open(path, errors="ignore").read().splitlines()
    assert lines[at - 1].rstrip() == old, (path, at, lines[at - 1])
