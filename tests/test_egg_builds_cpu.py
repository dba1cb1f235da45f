"""CPU tests of the definition of SBX_APP_EGG_STRAIGHT and SBX_APP_EGG_OVAL (include/sbx.h):
tests/egg_builds_model.py against the oracle (the shipped build, everything the three builds share) and against the frames and
points the reference header rendered with one line edited (tests/golden/egg_builds/, tools/make_golden_egg_builds.py); the
conditions on those fixtures; the model's sdf against the oracle's `egg.sdf` hook; and the name tables."""
import os
import subprocess

import numpy as np
import pytest

from tests import egg_builds_model as M
from tests.app_checks import assert_same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "egg_builds")
F = np.float32
NEW = ("straight", "oval")
MIN_PIXELS = {"straight": 90, "oval": 15}               # of a 96x54 frame, other than the shipped build's
MIN_POINTS = 200                                        # of the 4096 points


def golden(build):
    """(frames [(u_time, frame)], points [n, 2], their uniforms, the build's answers, the shipped build's answers) of one fixture"""
    z = np.load(os.path.join(GOLDEN, "egg_%s.npz" % build))
    keys = [k for k in z.files if k.startswith("t")]
    assert len(keys) == len(z["uniforms"]) == 3
    for k, u in zip(keys, z["uniforms"]):
        assert (u[0], u[1], u[2], u[3]) == (96, 54, 0, 0) and k == "t%g" % u[4]
        assert z[k].shape == (54, 96, 4) and z[k].dtype == np.float32
    assert z["points"].shape == (4096, 2) and z["points"].dtype == np.float32
    assert z["points_out"].shape == z["points_shipped"].shape == (4096, 4)
    assert tuple(z["points_uniforms"][:4]) == (1920, 1080, 0, 0)
    return [(float(u[4]), z[k]) for k, u in zip(keys, z["uniforms"])], z["points"], z["points_uniforms"], z["points_out"], z["points_shipped"]


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
        got = M.frame(build, 96, 54, t)
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
    assert [t for t, _ in frames] == [pytest.approx(x) for x in (0.0037, 0.02, 0.2)]
    for t, g in frames:
        n = int((~M.same_bits(g, oracle.render(APP_EGG, 96, 54, t)).all(axis=2)).sum())
        print(build, t, n)
        assert n >= MIN_PIXELS[build], (build, t, n)
    n = int((~M.same_bits(want, shipped).all(axis=1)).sum())
    print(build, "points", n)
    assert n >= MIN_POINTS, (build, n)
    assert (want[:, 3] == 1).all() and not np.isnan(want).any()
    assert os.path.getsize(os.path.join(GOLDEN, "egg_%s.npz" % build)) < 100 * 1024


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


# ---- names ---------------------------------------------------------------------------------------------------------------------

def test_python_names():
    import shaderbox_amd
    assert shaderbox_amd.APP_EGG_STRAIGHT == 19 == shaderbox_amd.ALL_APPS["APP_EGG_STRAIGHT"]
    assert shaderbox_amd.APP_EGG_OVAL == 20 == shaderbox_amd.ALL_APPS["APP_EGG_OVAL"]
    assert shaderbox_amd.app_id("egg_straight") == 19 and shaderbox_amd.app_id("egg_oval") == 20
    assert shaderbox_amd.app_id("APP_EGG_OVAL") == 20 and shaderbox_amd.app_id("egg") == 3
    # appended: no value renumbered.  (APPS itself keeps the nineteen apps before them: an existing test pins it to those.)
    assert sorted(shaderbox_amd.ALL_APPS.values()) == list(range(len(shaderbox_amd.ALL_APPS))) and len(shaderbox_amd.ALL_APPS) >= 21
    assert all(shaderbox_amd.ALL_APPS[k] == v for k, v in shaderbox_amd.APPS.items())
    assert shaderbox_amd.SBX_ABI_VERSION == 2


@pytest.mark.parametrize("defines,want", [(["APP_EGG_STRAIGHT"], "SBX_APP_EGG_STRAIGHT"), (["APP_EGG_OVAL"], "SBX_APP_EGG_OVAL"),
                                          (["APP_EGG", "APP_EGG_STRAIGHT"], "SBX_APP_EGG_STRAIGHT"),
                                          (["APP_EGG_OVAL", "APP_EGG"], "SBX_APP_EGG_OVAL"), (["APP_EGG"], "SBX_APP_EGG")])
def test_mainimage_header_selects_the_build(defines, want):
    r = subprocess.run(["g++", "-std=c++17", "-E", "-P", "-x", "c++"] + ["-D" + d for d in defines] +
                       ["-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "include", "sbx_mainimage.hpp")],
                       check=True, capture_output=True, text=True)
    assert "sbx_main_image(ctx, %s, &u" % want in r.stdout


def test_enum_values_of_the_header(tmp_path):
    src = tmp_path / "enum.cpp"
    src.write_text('#include "sbx.h"\nstatic_assert(SBX_APP_EGG == 3 && SBX_APP_SDF_AO_NORMALS == 18 && SBX_APP_EGG_STRAIGHT == 19 && '
                   'SBX_APP_EGG_OVAL == 20 && SBX_ABI_VERSION == 2, "appended");\n')
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)], check=True)
