"""CPU tests of the definition of SBX_APP_RAYTRACER_PHONG, SBX_APP_RAYTRACER_NOSHADOW and SBX_APP_RAYTRACER_STATIC (include/sbx.h,
DESIGN.md §5.14): tests/raytracer_builds_model.py against the oracle (the shipped build, everything the four builds share) and
against the frames and points the reference header rendered with one line edited (tests/golden/raytracer_builds/,
tools/make_golden_raytracer_builds.py); the conditions on those fixtures; and the name tables."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests import raytracer_builds_model as M
from tests.app_checks import assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "raytracer_builds")
NEW = ("phong", "noshadow", "static")
UNIFORMS = [(0.0, (0.0, 0.0)), (0.37, (0.0, 0.0)), (2.5, (0.0, 0.0)), (1.5, (40.0, 20.0))]      # (u_time, u_mouse) of the fixtures' frames
# caps that keep a fixture from saying nothing: pixels of a 4096-pixel frame / points of the 2048 other than the shipped build's
MIN_PIXELS = {"phong": 1500, "noshadow": 250, "static": 3500}
MIN_POINTS = {"phong": 500, "noshadow": 100, "static": 1500}


# ---- what the four builds share: the shipped build against the oracle ----------------------------------------------------------

@pytest.mark.parametrize("w,h", [(64, 64), (97, 55)])
def test_default_build_equals_the_oracle(oracle, w, h):
    from oracle.oracle import APP_RAYTRACER
    for t, mouse in UNIFORMS:
        got = M.frame("default", w, h, t, mouse)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_RAYTRACER, w, h, t, mouse=mouse), ("default", w, h, t, mouse))


# ---- the three other builds against the reference header's own frames and points -------------------------------------------------

@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_frames(build):
    frames = M.fixture(build)["frames"]
    assert [(t, m) for _, _, t, m, _ in frames] == [(pytest.approx(t), m) for t, m in UNIFORMS]
    for w, h, t, mouse, want in frames:
        assert (w, h) == (64, 64) and want.shape == (64, 64, 4) and want.dtype == np.float32
        assert_same(M.frame(build, w, h, t, mouse), want, (build, t, mouse))


@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_points(build):
    fx = M.fixture(build)
    pts, u = fx["points"], fx["points_uniforms"]
    assert pts.shape == (2048, 2) and pts.dtype == np.float32 and tuple(u) == (1920, 1080, 0, 0, 1.5)
    assert (pts != np.floor(pts) + .5).any(axis=1).all()                  # off-centre
    assert_same(M.main_image(build, u[0], u[1], u[4], pts[:, 0], pts[:, 1]), fx["points_out"], (build, "points"))
    assert_same(M.main_image("default", u[0], u[1], u[4], pts[:, 0], pts[:, 1]), fx["points_shipped"], (build, "the shipped build's answers"))


@pytest.mark.parametrize("build", NEW)
def test_fixture_conditions(oracle, build):
    """The fixtures tell the builds apart.  Measured: phong 2167, 2198, 2013 and 2944 pixels of the four 64x64 frames and 1407 of the
    2048 points; noshadow 533, 722, 392 and 604 pixels and 244 points; static 4040 pixels in every frame and 2030 points."""
    from oracle.oracle import APP_RAYTRACER
    fx = M.fixture(build)
    for w, h, t, mouse, g in fx["frames"]:
        assert not np.isnan(g).any() and (g[..., 3] == 1).all()
        n = int((~M.same_bits(g, oracle.render(APP_RAYTRACER, w, h, t, mouse=mouse)).all(axis=2)).sum())
        print(build, t, mouse, n)
        assert n >= MIN_PIXELS[build], (build, t, mouse, n)
    want, shipped = fx["points_out"], fx["points_shipped"]
    assert not np.isnan(want).any() and (want[:, 3] == 1).all()
    n = int((~M.same_bits(want, shipped).all(axis=1)).sum())
    print(build, "points", n)
    assert n >= MIN_POINTS[build], (build, n)
    if build == "static":                                                 # u_time is not read
        f = [g for _, _, _, mouse, g in fx["frames"] if mouse == (0.0, 0.0)]
        assert len(f) == 3 and M.same_bits(f[0], f[1]).all() and M.same_bits(f[0], f[2]).all()
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert os.path.getsize(os.path.join(GOLDEN, "raytracer_%s.npz" % build)) <= bound


def test_the_builds_differ_from_one_another():
    frames = {b: [g for *_, g in M.fixture(b)["frames"]] for b in NEW}
    for a, b in [("phong", "noshadow"), ("phong", "static"), ("noshadow", "static")]:
        for i in range(4):
            assert not M.same_bits(frames[a][i], frames[b][i]).all(), (a, b, i)
        assert not M.same_bits(M.fixture(a)["points_out"], M.fixture(b)["points_out"]).all(), (a, b, "points")


def test_static_build_reads_no_time():
    want = M.frame("static", 64, 64, 0.0)
    for t in (7.25, -1e30, float("inf"), float("nan")):
        assert_same(M.frame("static", 64, 64, t), want, ("static", t))
    assert not M.same_bits(M.frame("static", 64, 64, 0.0, (40.0, 20.0)), want).all()      # u_mouse still turns the camera


# ---- names ---------------------------------------------------------------------------------------------------------------------

def test_python_names():
    import shaderbox_amd
    for build, value in (("phong", 23), ("noshadow", 24), ("static", 25)):
        name = "APP_RAYTRACER_" + build.upper()
        assert getattr(shaderbox_amd, name) == value == shaderbox_amd.ALL_APPS[name] == shaderbox_amd.MORE_APPS[name]
        assert shaderbox_amd.app_id("raytracer_" + build) == value == shaderbox_amd.app_id(name)
        assert shaderbox_amd.app_id(M.APP_OF[build]) == value
    assert shaderbox_amd.app_id("raytracer") == 4 == shaderbox_amd.app_id("APP_RAYTRACER")
    # appended: no value renumbered, the table dense
    assert sorted(shaderbox_amd.ALL_APPS.values()) == list(range(len(shaderbox_amd.ALL_APPS))) and len(shaderbox_amd.ALL_APPS) >= 26
    assert all(shaderbox_amd.ALL_APPS[k] == v for k, v in shaderbox_amd.APPS.items())
    assert shaderbox_amd.SBX_ABI_VERSION == 2


def test_enum_lines_of_the_header(tmp_path):
    text = open(os.path.join(ROOT, "include", "sbx.h")).read()
    for line in ("    SBX_APP_RAYTRACER = 4,", "    SBX_APP_RAYTRACER_PHONG = 23,", "    SBX_APP_RAYTRACER_NOSHADOW = 24,",
                 "    SBX_APP_RAYTRACER_STATIC = 25", "#define SBX_ABI_VERSION 2"):
        assert sum(ln.split("/*")[0].rstrip() == line for ln in text.splitlines()) == 1, line
    src = tmp_path / "enum.cpp"
    src.write_text('#include "sbx.h"\nstatic_assert(SBX_APP_RAYTRACER == 4 && SBX_APP_CLOUDS_LUMINANCE == 22 && SBX_APP_RAYTRACER_PHONG == 23 && '
                   'SBX_APP_RAYTRACER_NOSHADOW == 24 && SBX_APP_RAYTRACER_STATIC == 25 && SBX_ABI_VERSION == 2, "appended");\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


@pytest.mark.parametrize("defines,want", [(["APP_RAYTRACER_PHONG"], "SBX_APP_RAYTRACER_PHONG"), (["APP_RAYTRACER_NOSHADOW"], "SBX_APP_RAYTRACER_NOSHADOW"),
                                          (["APP_RAYTRACER_STATIC"], "SBX_APP_RAYTRACER_STATIC"),
                                          (["APP_RAYTRACER", "APP_RAYTRACER_PHONG"], "SBX_APP_RAYTRACER_PHONG"),
                                          (["APP_RAYTRACER_NOSHADOW", "APP_RAYTRACER"], "SBX_APP_RAYTRACER_NOSHADOW"),
                                          (["APP_RAYTRACER", "APP_RAYTRACER_STATIC"], "SBX_APP_RAYTRACER_STATIC"),
                                          (["APP_RAYTRACER"], "SBX_APP_RAYTRACER")])
def test_mainimage_header_selects_the_build(defines, want):
    r = subprocess.run(["g++", "-std=c++17", "-E", "-P", "-x", "c++"] + ["-D" + d for d in defines] +
                       ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "sbx_mainimage.hpp")],
                       check=True, capture_output=True, text=True)
    assert "sbx_main_image(ctx, %s, &u" % want in r.stdout
