"""CPU tests of the definition of SBX_APP_VINYL_CLOSEUP, SBX_APP_VINYL_RIDGES and SBX_APP_VINYL_NOSHADOW (include/sbx.h,
DESIGN.md §5.15): tests/vinyl_builds_model.py against the oracle (the shipped build, everything the four builds share) and against
the frames and points the reference header rendered with one line edited (tests/golden/vinyl_builds/,
tools/make_golden_builds.py); and the conditions on those fixtures, which are tests/build_families.py's.  The name tables:
tests/test_build_families_cpu.py, which also asks every
family the header-selection cases at the end of this file."""
import glob
import os

import numpy as np
import pytest

from tests import vinyl_builds_model as M
from tests.app_checks import assert_same, check_mainimage_selects
from tests.build_families import FAMILIES, fixture_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = FAMILIES["vinyl"]
CAPS = FAMILY["builds"]                             # per build: the caps that keep a fixture from saying nothing (tests/build_families.py)
NEW = tuple(CAPS)
(W, H), (BW, BH) = FAMILY["size"], FAMILY["big"]["size"]
TIMES = tuple(t for t, _ in FAMILY["uniforms"])     # u_time of the fixtures' frames
BIG_TIMES = tuple(t for t, _ in FAMILY["big"]["uniforms"])      # u_time of the larger frames, of the builds that state a min_big
POINTS = FAMILY["points"]


def _differ(a, b):
    return int((~M.same_bits(a, b).all(axis=-1)).sum())


def _nan_pixels(a):
    return int(np.isnan(a).any(axis=-1).sum())


# ---- what the four builds share: the shipped build against the oracle ----------------------------------------------------------

@pytest.mark.parametrize("w,h,times", [(64, 36, (0.37, 2.5, -3.7)), (97, 55, (7.25,))])
def test_default_build_equals_the_oracle(oracle, w, h, times):
    from oracle.oracle import APP_VINYL
    for t in times:
        got = M.frame("default", w, h, t)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_VINYL, w, h, t), ("default", w, h, t))


# ---- the three other builds against the reference header's own frames and points -------------------------------------------------

@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_frames(build):
    fx = M.fixture(build)
    assert [tuple(u) for u in fx["uniforms"]] == [(W, H, 0, 0, np.float32(t)) for t in TIMES]
    for u, want in zip(fx["uniforms"], fx["frames"]):
        assert want.shape == (H, W, 4) and want.dtype == np.float32
        assert_same(M.frame(build, W, H, u[4]), want, (build, float(u[4])))
    big = [tuple(u) for u in fx["big_uniforms"]]
    assert big == ([(BW, BH, 0, 0, np.float32(t)) for t in BIG_TIMES] if "min_big" in CAPS[build] else [])
    for u, want in zip(fx["big_uniforms"], fx["big_frames"]):
        assert want.shape == (BH, BW, 4)
        assert_same(M.frame(build, BW, BH, u[4]), want, (build, "big", float(u[4])))


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
    """The fixtures tell the builds apart.  Measured, pixels other than the shipped build's in the 64x36 frames at u_time 0.37, 2.5,
    -3.7, 7.25 / the 128x72 frames at -3.7, 7.25 / the 2048 points: closeup 1541, 1545, 1548, 1531 / - / 1436; ridges 17, 92, 92,
    89 / 355, 345 / 92; noshadow 68, 67, 65, 66 / 254, 255 / 76.  NaN pixels: closeup 76, 71, 70, 66; ridges and noshadow 1, 2, 0,
    0 and 11, 14 at 128x72."""
    from oracle.oracle import APP_VINYL
    fx = M.fixture(build)
    for i, (u, g) in enumerate(zip(fx["uniforms"], fx["frames"])):
        assert (g[..., 3] == 1).all()
        n, nans = _differ(g, oracle.render(APP_VINYL, W, H, float(u[4]))), _nan_pixels(g)
        print(build, float(u[4]), n, "NaN pixels", nans)
        assert n >= np.broadcast_to(CAPS[build]["min_pixels"], len(TIMES))[i], (build, float(u[4]), n)
        assert nans <= CAPS[build]["max_nan"], (build, float(u[4]), nans)
    for u, g in zip(fx["big_uniforms"], fx["big_frames"]):
        assert (g[..., 3] == 1).all()
        n, nans = _differ(g, oracle.render(APP_VINYL, BW, BH, float(u[4]))), _nan_pixels(g)
        print(build, "big", float(u[4]), n, "NaN pixels", nans)
        assert n >= CAPS[build]["min_big"], (build, float(u[4]), n)
        assert nans <= CAPS[build]["max_nan_big"], (build, float(u[4]), nans)
    want, shipped = fx["points_out"], fx["points_shipped"]
    assert (want[:, 3] == 1).all() and (shipped[:, 3] == 1).all()
    n = _differ(want, shipped)
    print(build, "points", n)
    assert n >= CAPS[build]["min_points"], (build, n)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert FAMILY["max_bytes"] == "largest" and os.path.getsize(fixture_path(os.path.join(ROOT, "tests"), "vinyl", build)) <= bound


def test_the_builds_differ_from_one_another():
    frames = {b: M.fixture(b)["frames"] for b in NEW}
    for a, b in [("closeup", "ridges"), ("closeup", "noshadow"), ("ridges", "noshadow")]:
        for i in range(4):
            assert not M.same_bits(frames[a][i], frames[b][i]).all(), (a, b, i)
        assert not M.same_bits(M.fixture(a)["points_out"], M.fixture(b)["points_out"]).all(), (a, b, "points")


def test_closeup_differs_through_the_camera_only():
    """eye and look_at are the whole difference: the same sdf at the same points, the same hit block from the same hit"""
    assert M.CAMERA["closeup"] != M.CAMERA["default"] and M.CAMERA["ridges"] == M.CAMERA["noshadow"] == M.CAMERA["default"]
    rng = np.random.default_rng(5)
    pts = rng.uniform(-8, 8, size=(4096, 3)).astype(np.float32)
    pts[:, 1] = rng.uniform(-1, 3, size=4096).astype(np.float32)
    for t in (2.5, -3.7):
        a, b = M.sdf("closeup", t, *pts.T), M.sdf("default", t, *pts.T)
        assert M.same_bits(a[0], b[0]).all() and M.same_bits(a[1], b[1]).all()
        assert len({float(m) for m in a[1]}) >= 3                         # the points reach several members
    # the default build's render from the close-up camera's rays IS the close-up frame
    eye, look_at = M.CAMERA["closeup"]
    fx = (np.arange(64, dtype=np.float32) + np.float32(.5))[None, :]
    fy = (np.arange(36, dtype=np.float32) + np.float32(.5))[:, None]
    fx, fy = np.broadcast_arrays(fx, fy)
    pcx, pcy = M.point_cam(64, 36, fx.ravel(), fy.ravel(), M.FOV)
    rgb = M.render("default", 2.5, eye, M.get_primary_ray(pcx, pcy, eye, look_at))
    want = M.frame("closeup", 64, 36, 2.5)
    lin = M.oracle().math("pow", np.ascontiguousarray(rgb).ravel(), np.float32(1) / np.float32(2.2)).reshape(36, 64, 3)
    assert M.same_bits(lin, want[..., :3]).all()


def test_noshadow_is_the_lit_colour():
    """the model's `parts`: NOSHADOW's colour is illuminate's; the shipped build's is that times sh, equal wherever sh == 1"""
    pn, pd = {}, {}
    a = M.frame("noshadow", 64, 36, 2.5, parts=pn).reshape(-1, 4)
    b = M.frame("default", 64, 36, 2.5, parts=pd).reshape(-1, 4)
    assert (pn["sh"] == 1).all() and (pn["hit"] == pd["hit"]).all() and M.same_bits(pn["lit"], pd["lit"]).all()
    unshadowed = ~pd["hit"] | (pd["sh"] == 1)
    assert unshadowed.any() and (~unshadowed).any()
    assert M.same_bits(a[unshadowed], b[unshadowed]).all()


# ---- the app include/sbx_mainimage.hpp selects (every family's, from the table: tests/test_build_families_cpu.py) --------------------

@pytest.mark.parametrize("defines,want", [(["APP_VINYL_CLOSEUP"], "SBX_APP_VINYL_CLOSEUP"), (["APP_VINYL_RIDGES"], "SBX_APP_VINYL_RIDGES"),
                                          (["APP_VINYL_NOSHADOW"], "SBX_APP_VINYL_NOSHADOW"),
                                          (["APP_VINYL", "APP_VINYL_CLOSEUP"], "SBX_APP_VINYL_CLOSEUP"),
                                          (["APP_VINYL_RIDGES", "APP_VINYL"], "SBX_APP_VINYL_RIDGES"),
                                          (["APP_VINYL", "APP_VINYL_NOSHADOW"], "SBX_APP_VINYL_NOSHADOW"),
                                          (["APP_VINYL_NOSHADOW", "APP_VINYL"], "SBX_APP_VINYL_NOSHADOW"),
                                          (["APP_VINYL"], "SBX_APP_VINYL")])
def test_mainimage_header_selects_the_build(defines, want):
    check_mainimage_selects(defines, want)
