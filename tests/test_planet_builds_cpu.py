"""CPU tests of the definition of SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS and SBX_APP_PLANET_UNLIT (include/sbx.h,
DESIGN.md §5.16): tests/planet_builds_model.py against the oracle (the shipped build, everything the four builds share) and against
the frames and points the reference header rendered with one line edited (tests/golden/planet_builds/,
tools/make_golden_planet_builds.py); the conditions on those fixtures; and the name tables."""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests import planet_builds_model as M
from tests.app_checks import assert_same
from tests.model_common import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "planet_builds")
NEW = ("closeup", "cloudless", "unlit")
TIMES = (0.37, 2.5, -3.7, 7.25)                     # u_time of the fixtures' 64x36 frames
BIG_TIMES = (-3.7, 7.25)                            # u_time of the 128x72 frames (cloudless, unlit)
# caps that keep a fixture from saying nothing: pixels of a 64x36 frame and of a 128x72 frame other than the shipped build's; the most
# NaN pixels a frame may hold (the 0 / 0 of :273 is one source); and the points of the 2048 other than the shipped build's that
# tools/make_golden_planet_builds.py printed when it wrote the files (its docstring), of which 80 % are asked for
MIN_PIXELS = {"closeup": 2250, "cloudless": 750, "unlit": 580}
MIN_BIG = {"cloudless": 3000, "unlit": 2300}
MAX_NAN = {"closeup": 150, "cloudless": 100, "unlit": 0}
MAX_NAN_BIG = {"cloudless": 300, "unlit": 0}
PRINTED_POINTS = {"closeup": 2047, "cloudless": 796, "unlit": 659}


def _differ(a, b):
    return int((~same_bits(a, b).all(axis=-1)).sum())


def _nan_pixels(a):
    return int(np.isnan(a).any(axis=-1).sum())


# ---- what the four builds share: the shipped build against the oracle ----------------------------------------------------------

@pytest.mark.parametrize("w,h,times", [(64, 36, TIMES), (97, 55, (2.5,))])
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
    assert [tuple(u) for u in fx["uniforms"]] == [(64, 36, 0, 0, np.float32(t)) for t in TIMES]
    for u, want in zip(fx["uniforms"], fx["frames"]):
        assert want.shape == (36, 64, 4) and want.dtype == np.float32
        assert_same(M.frame(build, 64, 36, u[4]), want, (build, float(u[4])))
    big = [tuple(u) for u in fx["big_uniforms"]]
    assert big == ([(128, 72, 0, 0, np.float32(t)) for t in BIG_TIMES] if build in MIN_BIG else [])
    for u, want in zip(fx["big_uniforms"], fx["big_frames"]):
        assert want.shape == (72, 128, 4)
        assert_same(M.frame(build, 128, 72, u[4]), want, (build, "128x72", float(u[4])))


@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_points(build):
    fx = M.fixture(build)
    pts, u = fx["points"], fx["points_uniforms"]
    assert pts.shape == (2048, 2) and pts.dtype == np.float32 and tuple(u) == (1920, 1080, 0, 0, 2.5)
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
        n, nans = _differ(g, oracle.render(APP_PLANET, 64, 36, float(u[4]))), _nan_pixels(g)
        print(build, float(u[4]), n, "NaN pixels", nans)
        assert n >= MIN_PIXELS[build], (build, float(u[4]), n)
        assert nans <= MAX_NAN[build], (build, float(u[4]), nans)
    for u, g in zip(fx["big_uniforms"], fx["big_frames"]):
        assert (g[..., 3] == 1).all()
        n, nans = _differ(g, oracle.render(APP_PLANET, 128, 72, float(u[4]))), _nan_pixels(g)
        print(build, "128x72", float(u[4]), n, "NaN pixels", nans)
        assert n >= MIN_BIG[build], (build, float(u[4]), n)
        assert nans <= MAX_NAN_BIG[build], (build, float(u[4]), nans)
    want, shipped = fx["points_out"], fx["points_shipped"]
    assert (want[:, 3] == 1).all() and (shipped[:, 3] == 1).all()
    n = _differ(want, shipped)
    print(build, "points", n)
    assert n >= .8 * PRINTED_POINTS[build], (build, n)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    assert os.path.getsize(os.path.join(GOLDEN, "planet_%s.npz" % build)) <= bound


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


# ---- names ---------------------------------------------------------------------------------------------------------------------

def test_python_names():
    import shaderbox_amd
    for build, value in (("closeup", 29), ("cloudless", 30), ("unlit", 31)):
        name = "APP_PLANET_" + build.upper()
        assert getattr(shaderbox_amd, name) == value == shaderbox_amd.ALL_APPS[name] == shaderbox_amd.MORE_APPS[name]
        assert shaderbox_amd.app_id("planet_" + build) == value == shaderbox_amd.app_id(name)
        assert shaderbox_amd.app_id(M.APP_OF[build]) == value
        assert name not in shaderbox_amd.APPS
    assert shaderbox_amd.app_id("planet") == 0 == shaderbox_amd.app_id("APP_PLANET") and shaderbox_amd.app_id("planet_atmosphere") == 12
    # appended: no value renumbered, the table dense
    assert sorted(shaderbox_amd.ALL_APPS.values()) == list(range(len(shaderbox_amd.ALL_APPS))) and len(shaderbox_amd.ALL_APPS) >= 32
    assert all(shaderbox_amd.ALL_APPS[k] == v for k, v in shaderbox_amd.APPS.items())
    assert max(shaderbox_amd.APPS.values()) < 19 and len(shaderbox_amd.APPS) == 19          # APPS keeps its pinned entries
    assert shaderbox_amd.SBX_ABI_VERSION == 2


def test_enum_values_of_the_header(tmp_path):
    src = tmp_path / "enum.cpp"
    src.write_text('#include "sbx.h"\nstatic_assert(SBX_APP_PLANET == 0 && SBX_APP_PLANET_ATMOSPHERE == 12 && SBX_APP_VINYL_NOSHADOW == 28 && '
                   'SBX_APP_PLANET_CLOSEUP == 29 && SBX_APP_PLANET_CLOUDLESS == 30 && SBX_APP_PLANET_UNLIT == 31 && SBX_ABI_VERSION == 2, "appended");\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)


@pytest.mark.parametrize("defines,want", [(["APP_PLANET_CLOSEUP"], "SBX_APP_PLANET_CLOSEUP"), (["APP_PLANET_CLOUDLESS"], "SBX_APP_PLANET_CLOUDLESS"),
                                          (["APP_PLANET_UNLIT"], "SBX_APP_PLANET_UNLIT"),
                                          (["APP_PLANET", "APP_PLANET_CLOSEUP"], "SBX_APP_PLANET_CLOSEUP"),
                                          (["APP_PLANET_CLOUDLESS", "APP_PLANET"], "SBX_APP_PLANET_CLOUDLESS"),
                                          (["APP_PLANET", "APP_PLANET_UNLIT"], "SBX_APP_PLANET_UNLIT"),
                                          (["APP_PLANET_ATMOSPHERE"], "SBX_APP_PLANET_ATMOSPHERE"),
                                          (["APP_PLANET"], "SBX_APP_PLANET")])
def test_mainimage_header_selects_the_build(defines, want):
    r = subprocess.run(["g++", "-std=c++17", "-E", "-P", "-x", "c++"] + ["-D" + d for d in defines] +
                       ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "sbx_mainimage.hpp")],
                       check=True, capture_output=True, text=True)
    assert "sbx_main_image(ctx, %s, &u" % want in r.stdout
