"""CPU tests of the definition of SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval (include/sbx.h):
tests/atmosphere_air_model.py against the oracle's `atmosphere` frame (the default block, view 0), against
tests/atmosphere_ground_model.py (view 1), against the frames and points the reference header itself rendered with the four fixture
blocks written into it (tests/golden/atmosphere_airs/, tools/make_golden_atmosphere_airs.py) and, over default solver numbers,
against tests/atmosphere_eval_model.py on its four ray families; the conditions on those fixtures; the block
sbx_atmosphere_air_default returns; the table of tiers."""
import ctypes
import os

import numpy as np
import pytest

from tests import atmosphere_air_model as M
from tests import atmosphere_eval_model as E
from tests import atmosphere_ground_model as G
from tests.app_checks import assert_same

F = np.float32
W, H = M.SIZE
TIMES = E.TIMES                                     # five u_time


@pytest.mark.parametrize("w,h", [(64, 36), (97, 61)])
def test_default_block_equals_the_oracle_and_the_ground_model(oracle, w, h):
    from oracle.oracle import APP_IDS
    for t in TIMES:
        got = M.frame(M.default_air(t), w, h)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_IDS["atmosphere"], w, h, t), ("view 0", w, h, t))
        assert_same(M.frame(M.default_air(t, 1), w, h), G.frame(w, h, t), ("view 1", w, h, t))


def test_block_layout_and_the_librarys_default():
    """sbx_atmosphere_air_default (host code, no GPU): the model's default_air in every bit; the block is 128 bytes"""
    import shaderbox_amd
    assert ctypes.sizeof(shaderbox_amd.AtmosphereAir) == 128 and [n for n, _ in shaderbox_amd.AtmosphereAir._fields_] == list(M.FIELDS)
    for t in (0.0, .37, 2.5, -0.41, 1e9, float("nan")):
        for view in (0, 1):
            a = shaderbox_amd.atmosphere_air_default(t, view)
            assert np.array_equal(np.frombuffer(bytes(a), dtype=np.uint32), M.block(M.default_air(t, view))) or np.isnan(t), (t, view)
            assert_same(np.frombuffer(bytes(a), dtype=F)[4:], M.block(M.default_air(t, view)).view(F)[4:], ("sbx_atmosphere_air_default", t, view))
            assert (a.view, a.num_samples, a.num_samples_light, a.reserved0) == (view, 16, 8, 0)
    A = M.AIRS["thin"]
    b = shaderbox_amd.atmosphere_air(0., **{k: (list(map(float, A[k])) if isinstance(A[k], tuple) else float(A[k])) for k in
                                            ("earth_radius", "atmosphere_radius", "hR", "hM", "betaR", "betaM", "sun_power", "sun_dir", "eye")})
    assert np.array_equal(np.frombuffer(bytes(b), dtype=np.uint32), M.block(A)), "atmosphere_air"
    assert M.of_block(M.block(A)).keys() == A.keys() and np.array_equal(M.block(M.of_block(M.block(A))), M.block(A))


@pytest.mark.parametrize("name", sorted(M.AIRS))
def test_model_equals_the_reference_fixture(name):
    z = M.fixture(name)
    assert set(z.files) == {"block", "frame", "points", "points_out"}
    assert np.array_equal(z["block"], M.block(M.AIRS[name])), (name, "block")
    assert z["frame"].shape == (H, W, 4) and z["points"].shape == (M.POINTS, 2) and z["points_out"].shape == (M.POINTS, 4)
    assert_same(z["points"], M.fixture_points(M.POINT_SEEDS[name], W, H, M.POINTS), (name, "points"))
    assert not (z["points"] - np.floor(z["points"]) == .5).all(axis=1).any()
    assert_same(M.frame(M.AIRS[name], W, H), z["frame"], (name, "frame"))
    assert_same(M.points(M.AIRS[name], W, H, z["points"]), z["points_out"], (name, "points_out"))
    bound = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN) if f.endswith(".npz"))
    assert os.path.getsize(os.path.join(M.GOLDEN, "atmosphere_airs", "%s_%dx%d.npz" % (name, W, H))) <= bound


def test_fixture_conditions(oracle):
    """re-asserted of the committed files: lit sky, difference from the default block's frame of u_time .37, aloft's ground"""
    from oracle.oracle import APP_IDS
    frames = {n: M.fixture(n)["frame"] for n in M.AIRS}
    grounds = {n: M.ground_mask(A, W, H) for n, A in M.AIRS.items()}
    M.check_conditions(frames, grounds, oracle.render(APP_IDS["atmosphere"], W, H, .37))
    assert [M.refused(A) for A in M.AIRS.values()] == [None] * 4


@pytest.mark.parametrize("field", sorted(M.single_field_airs()))
def test_one_field_alone_changes_a_pixel(field):
    view, A = M.single_field_airs()[field]
    assert M.differing(M.frame(A, W, H), M.frame(M.default_air(.37, view), W, H)).any(), field


def test_look_at_is_not_read_by_view_0():
    assert_same(M.frame(M.air(.37, look_at=(1., 2., 3.)), W, H), M.frame(M.default_air(.37), W, H), "look_at, view 0")


def test_eval_model_with_default_solver_numbers_is_the_eval_model():
    """the four ray families of tests/atmosphere_eval_model.py; camera fields are not read"""
    rays = E.families()
    assert_same(M.get_sun_light(M.default_air(0.), rays), E.get_sun_light(rays), "get_sun_light")
    for s in E.SUNS[:3] + ((0.0, 2.0, 0.0),):
        A = M.air(0., sun_dir=s, view=1, eye=(1., 2., 3.), fov=7., look_at=(0., 0., 0.))
        assert_same(M.get_incident_light(A, rays), E.get_incident_light(rays, s), ("get_incident_light", s))


TIERS = [
    ("no change", M.default_air(.37), M.LITERAL),
    ("view 1", M.default_air(.37, 1), M.LITERAL),
    ("another sun", M.air(sun_dir=M.sun(2., 40.)), M.LITERAL),
    ("a NaN sun", M.air(sun_dir=(np.nan, 1., 0.)), M.LITERAL),
    ("view 1, fov and look_at", M.air(view=1, fov=1.3, look_at=(5., 6360e3, 2.)), M.LITERAL),
    ("view 0, fov", M.air(.37, fov=1.3), M.RUNTIME),
    ("view 0, look_at", M.air(.37, look_at=(5., 6360e3, 2.)), M.LITERAL),
    ("sun_power", M.air(.37, sun_power=19.), M.RUNTIME),
    ("hg_g NaN", M.air(.37, hg_g=np.nan), M.RUNTIME),
    ("betaR inf", M.air(.37, betaR=(np.inf, 1e-6, 1e-6)), M.RUNTIME),
    ("negative betaM", M.air(.37, betaM=(-1e-6, 1e-6, 1e-6)), M.RUNTIME),
    ("the eye", M.air(.37, eye=(0., 0., 0.)), M.RUNTIME),
    ("the eye, view 1", M.air(.37, 1, eye=(0., 6380e3, 0.)), M.RUNTIME),
    ("sun of length 2", M.air(sun_dir=(0., 2., 0.)), M.LITERAL),
    ("sun of length 2, sun_power", M.air(sun_dir=(0., 2., 0.), sun_power=19.), M.PLAIN),
    ("zero sun, sun_power", M.air(sun_dir=(0., 0., 0.), sun_power=19.), M.PLAIN),
    ("NaN sun, sun_power", M.air(sun_dir=(0., np.nan, 0.), sun_power=19.), M.PLAIN),
    ("sun at the edge of the class", M.air(sun_dir=(0., F(1.00004), 0.), sun_power=19.), M.RUNTIME),
    ("hR", M.air(.37, hR=7995.), M.PLAIN),
    ("hM = -0 next to it", M.air(.37, hM=-1200.), M.PLAIN),
    ("earth_radius", M.air(.37, earth_radius=6359e3), M.PLAIN),
    ("atmosphere_radius", M.air(.37, atmosphere_radius=6300e3), M.PLAIN),
    ("num_samples", M.air(.37, num_samples=15), M.PLAIN),
    ("num_samples_light", M.air(.37, num_samples_light=9), M.PLAIN),
    ("thin", M.AIRS["thin"], M.PLAIN), ("coarse", M.AIRS["coarse"], M.PLAIN), ("aloft", M.AIRS["aloft"], M.RUNTIME),
    ("sunset", M.AIRS["sunset"], M.LITERAL),
]


@pytest.mark.parametrize("what,A,want", TIERS, ids=[t[0] for t in TIERS])
def test_tier_of(what, A, want):
    assert M.tier_of(A) == want, what
    assert M.tier_of(A, variant=1) == M.PLAIN
    assert M.tier_of(A, variant=2) == want and M.tier_of(A, variant=3) == want
    assert M.tier_of(A, app=False) == (want if want != M.LITERAL else (M.RUNTIME if M.tame(A) else M.PLAIN))
    assert (want == M.RUNTIME) <= M.tame(A)


def test_refusals_of_the_model():
    assert M.refused(M.air(view=2)) == "view" and M.refused(M.air(view=-1)) == "view" and M.refused(M.air(view=2), app=False) is None
    assert M.refused(M.air(num_samples=0)) == M.refused(M.air(num_samples=65)) == "num_samples"
    assert M.refused(M.air(num_samples_light=0)) == M.refused(M.air(num_samples_light=33)) == "num_samples_light"
    assert M.refused(M.air(num_samples=64, num_samples_light=32)) is None and M.refused(M.air(num_samples=1, num_samples_light=1)) is None
    assert M.refused(M.air(reserved0=1)) == "reserved" and M.refused(M.air(reserved=(0., 0., 0., -0., 0., 0.))) == "reserved"
