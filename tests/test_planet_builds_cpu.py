"""CPU tests of the definition of SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS and SBX_APP_PLANET_UNLIT (include/sbx.h,
DESIGN.md §5.16): tests/planet_builds_model.py against the oracle (the shipped build, everything the four builds share) and against
the frames and points the reference header rendered with one line edited (tests/golden/planet_builds/,
tools/make_golden_builds.py); and the conditions on those fixtures, which are tests/build_families.py's.  The name tables:
tests/test_build_families_cpu.py, which also asks every
family the header-selection cases at the end of this file."""
import glob
import os

import numpy as np
import pytest

from tests import planet_builds_model as M
from tests.app_checks import assert_same, check_mainimage_selects
from tests.build_families import FAMILIES, fixture_path
from tests.model_common import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = FAMILIES["planet"]
CAPS = FAMILY["builds"]                             # per build: the caps that keep a fixture from saying nothing (tests/build_families.py)
NEW = tuple(CAPS)
(W, H), (BW, BH) = FAMILY["size"], FAMILY["big"]["size"]
TIMES = tuple(t for t, _ in FAMILY["uniforms"])     # u_time of the fixtures' frames
BIG_TIMES = tuple(t for t, _ in FAMILY["big"]["uniforms"])      # u_time of the larger frames, of the builds that state a min_big
POINTS = FAMILY["points"]


def _differ(a, b):
    return int((~same_bits(a, b).all(axis=-1)).sum())


def _nan_pixels(a):
    return int(np.isnan(a).any(axis=-1).sum())


# ---- what the four builds share: the shipped build against the oracle ----------------------------------------------------------

@pytest.mark.parametrize("w,h,times", [(W, H, TIMES), (97, 55, (2.5,))])
def test_default_build_equals_the_oracle(oracle, w, h, times):
    from oracle.oracle import APP_PLANET
    for t in times:
        got = M.frame("default", w, h, t)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_PLANET, w, h, t), ("default", w, h, t))


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
    -3.7, 7.25 / the 128x72 frames at -3.7, 7.25 / the 2048 points: closeup 2304 each / - / 2047; cloudless 873, 842, 885, 865 /
    3468, 3451 / 796; unlit 672, 684, 649, 665 / 2583, 2662 / 659.  NaN pixels: closeup 9, 32, 88, 12; cloudless 25, 21, 50, 20 and
    212, 75 at 128x72; unlit none."""
    from oracle.oracle import APP_PLANET
    fx = M.fixture(build)
    for u, g in zip(fx["uniforms"], fx["frames"]):
        assert (g[..., 3] == 1).all()
        n, nans = _differ(g, oracle.render(APP_PLANET, W, H, float(u[4]))), _nan_pixels(g)
        print(build, float(u[4]), n, "NaN pixels", nans)
        assert n >= CAPS[build]["min_pixels"], (build, float(u[4]), n)
        assert nans <= CAPS[build]["max_nan"], (build, float(u[4]), nans)
    for u, g in zip(fx["big_uniforms"], fx["big_frames"]):
        assert (g[..., 3] == 1).all()
        n, nans = _differ(g, oracle.render(APP_PLANET, BW, BH, float(u[4]))), _nan_pixels(g)
        print(build, "big", float(u[4]), n, "NaN pixels", nans)
        assert n >= CAPS[build]["min_big"], (build, float(u[4]), n)
        assert nans <= CAPS[build]["max_nan_big"], (build, float(u[4]), nans)
    want, shipped = fx["points_out"], fx["points_shipped"]
    assert (want[:, 3] == 1).all() and (shipped[:, 3] == 1).all()
    n = _differ(want, shipped)
    print(build, "points", n)
    assert n >= .8 * CAPS[build]["printed_points"], (build, n)             # 80 % of what the fixture tool printed
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert FAMILY["max_bytes"] == "largest" and os.path.getsize(fixture_path(os.path.join(ROOT, "tests"), "planet", build)) <= bound


def test_the_builds_differ_from_one_another():
    frames = {b: M.fixture(b)["frames"] for b in NEW}
    for a, b in [("closeup", "cloudless"), ("closeup", "unlit"), ("cloudless", "unlit")]:
        for i in range(4):
            assert not same_bits(frames[a][i], frames[b][i]).all(), (a, b, i)
        assert not same_bits(M.fixture(a)["points_out"], M.fixture(b)["points_out"]).all(), (a, b, "points")


def test_closeup_differs_through_the_camera_only():
    """eye and look_at are the whole difference: the default build's render from the close-up camera's rays IS the close-up frame"""
    assert M.CAMERA["closeup"] != M.CAMERA["default"] and M.CAMERA["cloudless"] == M.CAMERA["unlit"] == M.CAMERA["default"]
    eye, look_at = M.CAMERA["closeup"]
    fx = (np.arange(64, dtype=np.float32) + np.float32(.5))[None, :]
    fy = (np.arange(36, dtype=np.float32) + np.float32(.5))[:, None]
    fx, fy = np.broadcast_arrays(fx, fy)
    pcx, pcy = M.point_cam(64, 36, fx.ravel(), fy.ravel(), M.fov())
    rgb = M.render("default", 2.5, eye, M.get_primary_ray(pcx, pcy, eye, look_at))
    want = M.frame("closeup", 64, 36, 2.5)
    lin = M.oracle().math("pow", np.ascontiguousarray(rgb).ravel(), np.float32(1) / np.float32(2.2)).reshape(36, 64, 3)
    assert same_bits(lin, want[..., :3]).all()


@pytest.mark.parametrize("w,h,t", [(64, 36, 2.5), (97, 55, -3.7)])
def test_cloudless_is_the_shipped_build_where_no_cloud_enters(w, h, t):
    """the model's `parts`: where the shipped build's view march leaves cloud.alpha exactly 0 and the shadow is exactly 1 (the sky
    pixels among them: no ground hit, shadow never set), mix(x, radiance, 0) is x * 1 + radiance * 0 — the cloudless build's
    x * 1 + 0 * 0.  Such pixels exist, and so do pixels of the other kind."""
    pc, pd = {}, {}
    a = M.frame("cloudless", w, h, t, parts=pc).reshape(-1, 4)
    b = M.frame("default", w, h, t, parts=pd).reshape(-1, 4)
    assert (pc["alpha"] == 0).all() and (pc["shadow"] == 1).all()
    assert (pc["atm"] == pd["atm"]).all() and (pc["ground"] == pd["ground"]).all()
    clear = (pd["alpha"] == 0) & (pd["shadow"] == 1)
    assert (clear & pd["ground"]).any() and (clear & pd["atm"] & ~pd["ground"]).any() and (~clear).any() and (~pd["atm"]).any()
    assert same_bits(a[clear], b[clear]).all()
    assert not same_bits(a[~clear], b[~clear]).all()


def test_unlit_is_the_shipped_build_off_the_ground():
    """LIGHT enters illuminate alone: without a ground hit the two builds run the same statements"""
    pu, pd = {}, {}
    a = M.frame("unlit", 64, 36, 2.5, parts=pu).reshape(-1, 4)
    b = M.frame("default", 64, 36, 2.5, parts=pd).reshape(-1, 4)
    assert all(same_bits(pu[k].astype(np.float32), pd[k].astype(np.float32)).all() for k in ("atm", "ground", "alpha", "shadow"))
    sky = ~pd["ground"]
    assert sky.any() and (~sky).any()
    assert same_bits(a[sky], b[sky]).all() and not same_bits(a[~sky], b[~sky]).all()
    assert not np.isnan(a).any()


# ---- the app include/sbx_mainimage.hpp selects (every family's, from the table: tests/test_build_families_cpu.py) --------------------

@pytest.mark.parametrize("defines,want", [(["APP_PLANET_CLOSEUP"], "SBX_APP_PLANET_CLOSEUP"), (["APP_PLANET_CLOUDLESS"], "SBX_APP_PLANET_CLOUDLESS"),
                                          (["APP_PLANET_UNLIT"], "SBX_APP_PLANET_UNLIT"),
                                          (["APP_PLANET", "APP_PLANET_CLOSEUP"], "SBX_APP_PLANET_CLOSEUP"),
                                          (["APP_PLANET_CLOUDLESS", "APP_PLANET"], "SBX_APP_PLANET_CLOUDLESS"),
                                          (["APP_PLANET", "APP_PLANET_UNLIT"], "SBX_APP_PLANET_UNLIT"),
                                          (["APP_PLANET_ATMOSPHERE"], "SBX_APP_PLANET_ATMOSPHERE"),
                                          (["APP_PLANET"], "SBX_APP_PLANET")])
def test_mainimage_header_selects_the_build(defines, want):
    check_mainimage_selects(defines, want)
