"""CPU tests of the definition of SBX_APP_EGG_POSE and sbx_egg_eval (include/sbx.h): tests/egg_pose_model.py against
the oracle (the shipped pose: everything but the eight values of the block), against the oracle's `egg.sdf` hook, and against the
frames and points the reference header itself rendered with the four fixture poses written into it (tests/golden/egg_poses/,
tools/make_golden_egg_poses.py); the conditions on those fixtures; the block sbx_egg_pose_default returns; the solver's edge cases."""
import ctypes
import os

import numpy as np
import pytest

from tests import egg_pose_model as M
from tests.app_checks import assert_same, frame_cache

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
W, H = M.SIZE

shares_of = frame_cache(lambda name: M.shares(M.scene_of(M.POSES[name]), W, H))


@pytest.mark.parametrize("w,h", [(64, 64), (64, 36)])
def test_default_pose_equals_the_oracle(oracle, w, h):
    from oracle.oracle import APP_EGG
    for t in (0.0, 1.3, 7.77):
        got = M.frame(M.scene_of(M.default_pose(t)), w, h)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_EGG, w, h, t), ("default pose", w, h, t))


def test_default_pose_equals_the_golden_frame():
    """tests/golden/egg_64x64.npz as tests/test_golden.py reads it"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "egg_64x64.npz"))
    assert len(z.files) >= 3
    for key in z.files:                              # "t<u_time>"
        assert_same(M.frame(M.scene_of(M.default_pose(float(key[1:]))), 64, 64), z[key], ("golden egg frame", key))


def test_default_block_is_the_librarys():
    """sbx_egg_pose_default (host code, no GPU): the model's default_pose in every bit"""
    import shaderbox_amd
    for t in (0.0, 1.3, 7.77, -0.41, 1e9, float("nan")):
        a = shaderbox_amd.egg_pose_default(t)
        assert ctypes.sizeof(a) == 64
        got = np.frombuffer(bytes(a), dtype=F)
        assert_same(got, M.block(M.default_pose(t)), ("sbx_egg_pose_default", t))
    b = shaderbox_amd.egg_pose((.45, 1.25, .35), (-.3, 1.05, -.1), turn_deg=35., eye=(2., 1., 4.5), look_at=(0., 0., 0.), fov=.8)
    assert_same(np.frombuffer(bytes(b), dtype=F), M.block(M.POSES["stride"]), "egg_pose")


def test_sdf_equals_the_oracles_hook(oracle):
    rng = np.random.default_rng(7)
    for t in (0.02, 1.3):
        S = M.scene_of(M.default_pose(t))
        p = np.concatenate([rng.uniform(-2, 2, size=(800, 3)) + [0, 0, 3.5], rng.uniform(-30, 30, size=(100, 3)),
                            [[0, 0, 0], [0, 1.15, 3.5], [0, -1.7, 0], [np.nan, 1, 1], [np.inf, 1, 1], [1, -np.inf, 1], [1e30, -1e30, 3]]]).astype(F)
        d, m = M.sdf(S, p[:, 0], p[:, 1], p[:, 2])
        want = np.stack([oracle.kat("egg.sdf", [96, 54, 0, 0, t] + list(q), 2) for q in p])
        assert_same(np.stack([d, m], axis=1), want, ("sdf", t))


@pytest.mark.parametrize("name", sorted(M.POSES))
def test_model_equals_the_reference_fixture(name):
    z = M.fixture(name)
    assert set(z.files) == {"pose", "frame", "points", "points_out"}
    assert_same(z["pose"], M.block(M.POSES[name]), (name, "pose"))
    assert z["frame"].shape == (H, W, 4) and z["points"].shape == (M.POINTS, 2) and z["points_out"].shape == (M.POINTS, 4)
    assert_same(z["points"], M.fixture_points(M.POINT_SEEDS[name], W, H, M.POINTS), (name, "points"))
    assert_same(shares_of(name)[1], z["frame"], (name, "frame"))
    assert_same(M.points(M.scene_of(M.POSES[name]), W, H, z["points"]), z["points_out"], (name, "points_out"))
    assert os.path.getsize(os.path.join(M.GOLDEN, "egg_poses", "%s_%dx%d.npz" % (name, W, H))) < 1 << 20


def test_fixture_conditions():
    for name in M.POSES:
        print(name, {k: round(float(v), 4) for k, v in shares_of(name)[0].items()})
    M.check_conditions({n: shares_of(n)[0] for n in M.POSES}, {n: M.fixture(n)["frame"] for n in M.POSES})


def test_rays_of_a_frame_tie_render_scene_to_the_pixel():
    """render_scene over the primary rays, then render's bars, abs and sRGB: the frame"""
    P = M.POSES["stride"]
    S = M.scene_of(P)
    fx = (np.arange(W, dtype=F) + F(.5))[None, :]
    fy = (np.arange(H, dtype=F) + F(.5))[:, None]
    pcx, ro, rd = M.primary_rays(P, W, H, fx, fy)
    rgb, depth = M.render_scene(S, ro, rd)
    assert_same(M.finish(rgb, depth, pcx).reshape(H, W, 4), M.fixture("stride")["frame"], "render_scene + finish")


def ik(start, goal, l1, l2):
    with np.errstate(all="ignore"):
        return np.array(M.ik_solver(tuple(map(F, start)), tuple(map(F, goal)), F(l1), F(l2)), dtype=F)


def test_ik_solver_edge_cases():
    """IK.h:18-41 as the arithmetic says: what is a NaN, what is finite"""
    # a reachable goal: the knee is L1 from the start and L2 from the goal
    k = ik((0, 0, .2), (.1, 1.2, .2), .8, .75).astype(np.float64)
    assert abs(np.linalg.norm(k - [0, 0, .2]) - .8) < 1e-6 and abs(np.linalg.norm(k - [.1, 1.2, .2]) - .75) < 1e-5
    # goal = start: G = 0, cos_theta = (L1^2 - L2^2) / 0 is an inf, sin_theta a NaN, normalize(0) a NaN: a NaN knee
    assert np.isnan(ik((0, 0, .2), (0, 0, .2), .8, .75)).all()
    # L1 = 0: cos_theta = (G^2 - L2^2) / 0, an inf (or 0 / 0): NaN in x and y; z = start.z + (0 + 0) + n.z * 0 is finite
    k = ik((0, 0, .2), (0, 1, .2), 0., .75)
    assert np.isnan(k[:2]).all() and k[2] == F(.2)
    # G = L1 + L2 exactly (1 + .5): cos_theta = 1, sin_theta = 0, the knee on the line to the goal, finite
    k = ik((0, 0, 0), (0, 1.5, 0), 1., .5)
    assert_same(k, np.array([0, 1, 0], dtype=F), "straight leg")
    # unreachable (beyond L1 + L2) and folded (inside |L1 - L2|): |cos_theta| > 1, sqrt of a negative: NaN in x and y
    assert np.isnan(ik((0, 0, 0), (0, 2, 0), .8, .75)[:2]).all()
    assert np.isnan(ik((0, 0, 0), (0, .1, 0), 1., .5)[:2]).all()
    # a goal off the pelvis' z plane: a 3-D goal rotated about z, z carried through mul's last column
    k = ik((0, 0, .2), (.3, 1., -.1), .8, .75)
    assert np.isfinite(k).all()
    # the fixture pose `reach`: the left knee is a NaN, the right one is not
    S = M.scene_of(M.POSES["reach"])
    assert np.isnan(np.array(S["knee_l"])).any() and np.isfinite(np.array(S["knee_r"])).all()
