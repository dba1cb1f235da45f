"""CPU tests of the definition of SBX_APP_EGG_STRAIGHT and SBX_APP_EGG_OVAL (include/sbx.h):
tests/egg_builds_model.py against the oracle (the shipped build, everything the three builds share) and against the frames and
points the reference header rendered with one line edited (tests/golden/egg_builds/, tools/make_golden_builds.py); the
conditions on those fixtures, which are tests/build_families.py's; and the model's sdf against the oracle's `egg.sdf` hook.  The name
tables: tests/test_build_families_cpu.py, which also asks every
family the header-selection cases at the end of this file."""
import os

import numpy as np
import pytest

from tests import egg_builds_model as M
from tests.app_checks import assert_same, check_mainimage_selects
from tests.build_families import FAMILIES, fixture_path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FAMILY = FAMILIES["egg"]
CAPS = FAMILY["builds"]                             # per build: the caps that keep a fixture from saying nothing (tests/build_families.py)
NEW = tuple(CAPS)
W, H = FAMILY["size"]
POINTS = FAMILY["points"]


def golden(build):
    """(frames [(u_time, frame)], points [n, 2], their uniforms, the build's answers, the shipped build's answers) of one fixture"""
    z = M.fixture(build)                            # (which asserts the file's keys and uniforms to be the table's)
    assert len(z["frames"]) == len(z["uniforms"]) == len(FAMILY["uniforms"])
    for f, u in zip(z["frames"], z["uniforms"]):
        assert (u[0], u[1], u[2], u[3]) == (W, H, 0, 0)
        assert f.shape == (H, W, 4) and f.dtype == np.float32
    assert z["points"].shape == (POINTS["count"], 2) and z["points"].dtype == np.float32
    assert z["points_out"].shape == z["points_shipped"].shape == (POINTS["count"], 4)
    assert tuple(z["points_uniforms"][:4]) == POINTS["size"] + (0, 0)
    return [(float(u[4]), f) for f, u in zip(z["frames"], z["uniforms"])], z["points"], z["points_uniforms"], z["points_out"], z["points_shipped"]


# ---- what the three builds share: the shipped build against the oracle --------------------------------------------------------

@pytest.mark.parametrize("w,h", [(64, 64), (257, 130)])
def test_default_build_equals_the_oracle(oracle, w, h):
    from oracle.oracle import APP_EGG
    for t in (0.0, 0.0037, 0.2, 0.37, -0.41, 1.3, 100.5):
        got = M.frame("default", w, h, t)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_EGG, w, h, t), ("default", w, h, t))


def test_default_build_points_equal_the_oracle(oracle):
    from oracle.oracle import APP_EGG
    w, h, t = 1920, 1080, 0.02
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(0, 1, size=(150, 2)) * [w, h], rng.uniform(-3, 4, size=(80, 2)) * [w, h],
                          [[0, 0], [w, h], [-.5, -.5], [1e30, 1e30], [-3e38, 5], [np.inf, 5], [5, -np.inf], [np.nan, 5], [np.nan, np.nan]]]).astype(F)
    want = np.stack([oracle.main_image(APP_EGG, w, h, t, x, y) for x, y in pts])
    assert_same(M.main_image("default", w, h, t, pts[:, 0], pts[:, 1]), want, "points")


def test_sdf_equals_the_oracles_hook(oracle):
    """the oracle exposes sdf() of the shipped build (`egg.sdf`): the model's, at random points, at hits of a frame and at
    non-finite points; and every member of the union wins somewhere"""
    rng = np.random.default_rng(7)
    for t in (0.02, -0.41):
        parts = {}
        fx = (np.arange(96, dtype=F) + F(.5))[None, :]
        fy = (np.arange(54, dtype=F) + F(.5))[:, None]
        M.main_image("default", 96, 54, t, fx, fy, parts=parts)
        hits = parts["p"][parts["hit"]]
        assert set(np.unique(parts["mat"][parts["hit"]])) == {1, 2, 3}
        p = np.concatenate([rng.uniform(-2, 2, size=(1200, 3)) + [0, 0, 3.5], rng.uniform(-30, 30, size=(200, 3)), hits[::4],
                            [[0, 0, 0], [0, 1.15, 3.5], [0, -1.7, 0], [np.nan, 1, 1], [np.inf, 1, 1], [1, -np.inf, 1], [1e30, -1e30, 3]]]).astype(F)
        d, m = M.sdf("default", t, p[:, 0], p[:, 1], p[:, 2])
        want = np.stack([oracle.kat("egg.sdf", [96, 54, 0, 0, t] + list(q), 2) for q in p])
        assert_same(np.stack([d, m], axis=1), want, ("sdf", t))
        assert set(np.unique(m)) == {1, 2, 3}


# ---- the two other builds against the reference header's own frames and points --------------------------------------------------

@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_frames(build):
    for t, want in golden(build)[0]:
        got = M.frame(build, W, H, t)
        assert not np.isnan(want).any()
        assert_same(got, want, (build, t))


@pytest.mark.parametrize("build", NEW)
def test_builds_equal_the_reference_points(build):
    _, pts, u, want, shipped = golden(build)
    assert_same(M.main_image(build, u[0], u[1], u[4], pts[:, 0], pts[:, 1]), want, (build, "points"))
    assert_same(M.main_image("default", u[0], u[1], u[4], pts[:, 0], pts[:, 1]), shipped, (build, "the shipped build's answers"))


@pytest.mark.parametrize("build", NEW)
def test_fixture_conditions(oracle, build):
    """The fixtures tell the builds apart.  Measured: straight 128, 135 and 100 pixels of the 96x54 frames at u_time 0.0037, 0.02
    and 0.2 and 985 of the 4096 points; oval 20, 21 and 20 pixels and 297 points."""
    from oracle.oracle import APP_EGG
    frames, pts, u, want, shipped = golden(build)
    assert [t for t, _ in frames] == [pytest.approx(x) for x, _ in FAMILY["uniforms"]]
    for t, g in frames:
        n = int((~M.same_bits(g, oracle.render(APP_EGG, W, H, t)).all(axis=2)).sum())
        print(build, t, n)
        assert n >= CAPS[build]["min_pixels"], (build, t, n)
    n = int((~M.same_bits(want, shipped).all(axis=1)).sum())
    print(build, "points", n)
    assert n >= CAPS[build]["min_points"], (build, n)
    assert (want[:, 3] == 1).all() and FAMILY["no_nan"] and not np.isnan(want).any()
    x0, y0, x1, y1 = CAPS[build]["rect"]
    assert ((pts >= (x0, y0)) & (pts <= (x1, y1))).all()
    assert os.path.getsize(fixture_path(os.path.join(ROOT, "tests"), "egg", build)) < FAMILY["max_bytes"]


def test_what_the_builds_change():
    """straight: only the legs' field differs from the shipped build's; oval: only the egg's, which is never above the sphere of
    radius .475 * 1.55 around (0, .65, 0) divided by 1.55 (the bound k_egg's cull uses, kern_egg.hip)"""
    rng = np.random.default_rng(3)
    p = (rng.uniform(-2, 2, size=(4000, 3)) + [0, 0, 3.5]).astype(F)
    for t in (0.02, 0.2):
        ref, got = {}, {}
        M.sdf("default", t, p[:, 0], p[:, 1], p[:, 2], members=ref)
        M.sdf("straight", t, p[:, 0], p[:, 1], p[:, 2], members=got)
        for k in ("egg", "feet", "bike", "ground"):
            assert_same(got[k], ref[k], ("straight", k))
        assert not M.same_bits(got["legs"], ref["legs"]).all()
        got = {}
        M.sdf("oval", t, p[:, 0], p[:, 1], p[:, 2], members=got)
        for k in ("legs", "feet", "bike", "ground"):
            assert_same(got[k], ref[k], ("oval", k))
        assert not M.same_bits(got["egg"], ref["egg"]).all()
        S = M.scene(t)
        r = M.mat_vec(S["rot_y"], (p[:, 0], p[:, 1], p[:, 2]))
        q = np.sqrt(r[0].astype(np.float64) ** 2 + (r[1].astype(np.float64) - 0.5 - 0.65) ** 2 + (r[2].astype(np.float64) - 3.5) ** 2)
        assert (got["egg"] >= q / 1.5501 - 0.475 - 1e-6).all()


# ---- the app include/sbx_mainimage.hpp selects (every family's, from the table: tests/test_build_families_cpu.py) --------------------

@pytest.mark.parametrize("defines,want", [(["APP_EGG_STRAIGHT"], "SBX_APP_EGG_STRAIGHT"), (["APP_EGG_OVAL"], "SBX_APP_EGG_OVAL"),
                                          (["APP_EGG", "APP_EGG_STRAIGHT"], "SBX_APP_EGG_STRAIGHT"),
                                          (["APP_EGG_OVAL", "APP_EGG"], "SBX_APP_EGG_OVAL"), (["APP_EGG"], "SBX_APP_EGG")])
def test_mainimage_header_selects_the_build(defines, want):
    check_mainimage_selects(defines, want)
