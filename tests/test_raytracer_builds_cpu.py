"""CPU tests of the definition of SBX_APP_RAYTRACER_PHONG, SBX_APP_RAYTRACER_NOSHADOW and SBX_APP_RAYTRACER_STATIC (include/sbx.h,
DESIGN.md §5.14): tests/raytracer_builds_model.py against the oracle (the shipped build, everything the four builds share) and
against the frames and points the reference header rendered with one line edited (tests/golden/raytracer_builds/,
tools/make_golden_builds.py); and the conditions on those fixtures, which are tests/build_families.py's.  The name tables:
tests/test_build_families_cpu.py, which also asks every
family the header-selection cases at the end of this file."""
import glob
import os

import numpy as np
import pytest

from tests import raytracer_builds_model as M
from tests.app_checks import assert_same, check_mainimage_selects
from tests.build_families import FAMILIES, fixture_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = FAMILIES["raytracer"]
CAPS = FAMILY["builds"]                             # per build: the caps that keep a fixture from saying nothing (tests/build_families.py)
NEW = tuple(CAPS)
W, H = FAMILY["size"]
UNIFORMS = list(FAMILY["uniforms"])                 # (u_time, u_mouse) of the fixtures' frames
POINTS = FAMILY["points"]


# ---- what the four builds share: the shipped build against the oracle ----------------------------------------------------------

@pytest.mark.parametrize("w,h", [(W, H), (97, 55)])
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
        assert (w, h) == (W, H) and want.shape == (H, W, 4) and want.dtype == np.float32
        assert_same(M.frame(build, w, h, t, mouse), want, (build, t, mouse))


@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_points(build):
    fx = M.fixture(build)
    pts, u = fx["points"], fx["points_uniforms"]
    assert pts.shape == (POINTS["count"], 2) and pts.dtype == np.float32 and tuple(u) == POINTS["size"] + (0, 0, POINTS["time"])
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
        assert n >= CAPS[build]["min_pixels"], (build, t, mouse, n)
    want, shipped = fx["points_out"], fx["points_shipped"]
    assert not np.isnan(want).any() and (want[:, 3] == 1).all()
    n = int((~M.same_bits(want, shipped).all(axis=1)).sum())
    print(build, "points", n)
    assert n >= CAPS[build]["min_points"], (build, n)
    assert ("equal_frames" in CAPS[build]) == (build == "static")
    if build == "static":                                                 # u_time is not read
        f = [g for _, _, _, mouse, g in fx["frames"] if mouse == (0.0, 0.0)]
        assert len(f) == 3 and M.same_bits(f[0], f[1]).all() and M.same_bits(f[0], f[2]).all()
        assert [fx["frames"][i][3] for i in CAPS[build]["equal_frames"]] == [(0.0, 0.0)] * 3
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert FAMILY["max_bytes"] == "largest" and os.path.getsize(fixture_path(os.path.join(ROOT, "tests"), "raytracer", build)) <= bound


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


# ---- the app include/sbx_mainimage.hpp selects (every family's, from the table: tests/test_build_families_cpu.py) --------------------

@pytest.mark.parametrize("defines,want", [(["APP_RAYTRACER_PHONG"], "SBX_APP_RAYTRACER_PHONG"), (["APP_RAYTRACER_NOSHADOW"], "SBX_APP_RAYTRACER_NOSHADOW"),
                                          (["APP_RAYTRACER_STATIC"], "SBX_APP_RAYTRACER_STATIC"),
                                          (["APP_RAYTRACER", "APP_RAYTRACER_PHONG"], "SBX_APP_RAYTRACER_PHONG"),
                                          (["APP_RAYTRACER_NOSHADOW", "APP_RAYTRACER"], "SBX_APP_RAYTRACER_NOSHADOW"),
                                          (["APP_RAYTRACER", "APP_RAYTRACER_STATIC"], "SBX_APP_RAYTRACER_STATIC"),
                                          (["APP_RAYTRACER"], "SBX_APP_RAYTRACER")])
def test_mainimage_header_selects_the_build(defines, want):
    check_mainimage_selects(defines, want)
