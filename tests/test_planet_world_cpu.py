"""CPU tests of the definition of SBX_APP_PLANET_WORLD (include/sbx.h): tests/planet_world_model.py against
tests/planet_builds_model.py's shipped frame (the default world; the oracle pins that one to the reference), against the frames and
points the reference header itself rendered with the five fixture worlds written into it (tests/golden/planet_worlds/,
tools/make_golden_planet_worlds.py); the conditions on those fixtures; the block sbx_planet_world_default returns; the refusals; the
single-field property; the table of tiers."""
import ctypes
import os

import numpy as np
import pytest

from tests import planet_builds_model as P
from tests import planet_world_model as M
from tests.app_checks import assert_same, frame_cache

F = np.float32
W, H = M.SIZE

default_frame = frame_cache(lambda t: M.frame(M.default_world(t), W, H))


@pytest.mark.parametrize("t", [0.0, .37, 2.5])
def test_default_world_is_the_shipped_frame(t):
    got = default_frame(t)
    assert (got[..., 3] == 1).all()
    assert_same(got, P.frame("default", W, H, t), ("64x36", t))


def test_default_world_shows_what_the_shipped_frame_shows():
    """the counts the issue of this app states for the shipped 64x36 frame at u_time .37; NaN pixels are data"""
    parts = {}
    f = M.frame(M.default_world(.37), W, H, parts)
    c = M.classes(parts, (H, W))
    assert (int(c["shell"].sum()), int(c["ground"].sum()), int(np.isnan(f).any(axis=-1).sum())) == (1304, 672, 25)
    assert_same(M.frame(M.default_world(.37), 97, 61), P.frame("default", 97, 61, .37), "97x61")


def test_block_layout_and_the_librarys_default():
    """sbx_planet_world_default (host code, no GPU): the model's default_world in every bit; the block is 224 bytes"""
    import shaderbox_amd
    assert ctypes.sizeof(shaderbox_amd.PlanetWorld) == 224 == 4 * M.WORDS and [n for n, _ in shaderbox_amd.PlanetWorld._fields_] == list(M.FIELDS)
    for t in (0.0, .37, 2.5, -0.41, 1e9, float("inf")):
        a = shaderbox_amd.planet_world_default(t)
        assert np.array_equal(np.frombuffer(bytes(a), dtype=np.uint32), M.block(M.default_world(t))), t
    a = shaderbox_amd.planet_world_default(float("nan"))
    assert np.isnan(a.spin_deg) and np.isnan(a.cloud_spin_deg) and a.tilt_deg == 27.0
    for name, Wd in M.WORLDS.items():
        D = M.default_world(M.T0)
        changed = {k: (Wd[k] if k in M.INT_FIELDS else list(map(float, Wd[k])) if isinstance(Wd[k], tuple) else float(Wd[k]))
                   for k in M.FIELDS if k != "reserved" and not np.array_equal(np.asarray(Wd[k]), np.asarray(D[k]))}
        b = shaderbox_amd.planet_world(M.T0, **changed)
        assert np.array_equal(np.frombuffer(bytes(b), dtype=np.uint32), M.block(Wd)), name
        assert np.array_equal(M.block(M.of_block(M.block(Wd))), M.block(Wd))
        assert np.array_equal(np.frombuffer(bytes(M.as_aux(Wd)), dtype=np.uint32), M.block(Wd))
    with pytest.raises(shaderbox_amd.SbxError):
        shaderbox_amd.planet_world(0., no_such_field=1.)


def test_every_field_differs_in_some_fixture_world():
    D = M.default_world(M.T0)
    for k in M.FIELDS:
        if k != "reserved":
            assert any(not np.array_equal(np.asarray(Wd[k]), np.asarray(D[k])) for Wd in M.WORLDS.values()), k


@pytest.mark.parametrize("name", sorted(M.WORLDS))
def test_model_equals_the_reference_fixture(name):
    z = M.fixture(name)
    assert set(z.files) == {"block", "frame", "points", "points_out"}
    assert np.array_equal(z["block"], M.block(M.WORLDS[name])), (name, "block")
    assert z["frame"].shape == (H, W, 4) and z["points"].shape == (M.POINTS, 2) and z["points_out"].shape == (M.POINTS, 4)
    assert_same(z["points"], M.fixture_points(M.POINT_SEEDS[name], W, H, M.POINTS), (name, "points"))
    assert not (z["points"] - np.floor(z["points"]) == .5).all(axis=1).any()
    assert_same(M.frame(M.WORLDS[name], W, H), z["frame"], (name, "frame"))
    assert_same(M.points(M.WORLDS[name], W, H, z["points"]), z["points_out"], (name, "points_out"))
    bound = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN) if f.endswith(".npz"))
    assert os.path.getsize(os.path.join(M.GOLDEN, "planet_worlds", "%s_%dx%d.npz" % (name, W, H))) <= bound


def test_fixture_conditions():
    """re-asserted of the committed files (the reference's frames): the four kinds of pixel, the difference from the default world's
    frame of u_time .37, the tiers"""
    frames = {n: M.fixture(n)["frame"] for n in M.WORLDS}
    parts_of = {}
    for n, Wd in M.WORLDS.items():
        parts_of[n] = {}
        M.frame(Wd, W, H, parts_of[n])
    M.check_conditions(frames, parts_of, default_frame(.37))
    assert [M.refused(Wd) for Wd in M.WORLDS.values()] == [None] * 5
    assert any(np.isnan(f).any() for f in frames.values()), "NaN pixels are data: the fixtures hold some"


@pytest.mark.parametrize("field", sorted(M.single_field_worlds()))
def test_one_field_alone_changes_a_pixel(field):
    assert M.differing(M.frame(M.single_field_worlds()[field], W, H), default_frame(.37)).any(), field


TIERS = [
    ("no change", M.default_world(.37), M.LITERAL),
    ("orbit", M.WORLDS["orbit"], M.LITERAL),
    ("another sun", M.world(.37, sun_dir=(0., 2., 0.)), M.LITERAL),
    ("a NaN sun", M.world(.37, sun_dir=(np.nan, 1., 0.)), M.LITERAL),
    ("a zero sun", M.world(.37, sun_dir=(0., 0., 0.)), M.LITERAL),
    ("an eye at the bound", M.world(.37, eye=(0., 256., 0.)), M.LITERAL),
    ("an eye beyond it", M.world(.37, eye=(0., 257., 0.)), M.PLAIN),
    ("a huge eye", M.world(.37, eye=(1e30, 0., 0.)), M.PLAIN),
    ("eye == look_at", M.world(.37, eye=(0., 0., 2.)), M.PLAIN),
    ("fov 0", M.world(.37, fov=0.), M.LITERAL),
    ("fov NaN", M.world(.37, fov=np.nan), M.PLAIN),
    ("inf spin", M.world(.37, spin_deg=np.inf), M.PLAIN),
    ("a spin beyond 1e9", M.world(.37, cloud_spin_deg=2e9), M.PLAIN),
    ("a NaN tilt", M.world(.37, tilt_deg=np.nan), M.PLAIN),
    ("one colour bit", M.world(.37, c_snow=(np.nextafter(F(.6), F(1)), .6, .6)), M.RUNTIME),
    ("NaN colour", M.world(.37, c_rock=(np.nan, 0., 0.)), M.RUNTIME),
    ("negative key light", M.world(.37, key_color=(-1., 0., 1e30)), M.RUNTIME),
    ("inf limit", M.world(.37, l_rock=np.inf), M.RUNTIME),
    ("a colour and a NaN sun", M.world(.37, c_rock=(.1, 0., 0.), sun_dir=(np.nan, 0., 0.)), M.RUNTIME),
    ("a colour and a huge eye", M.world(.37, c_rock=(.1, 0., 0.), eye=(1e30, 0., 0.)), M.RUNTIME),     # the wave's business, not the host's
    ("a colour and eye == look_at", M.world(.37, c_rock=(.1, 0., 0.), eye=(0., 0., 2.)), M.RUNTIME),
    ("a colour and an inf spin", M.world(.37, c_rock=(.1, 0., 0.), spin_deg=np.inf), M.PLAIN),
    ("max_height 0", M.world(.37, max_height=0.), M.PLAIN),
    ("max_height negative", M.world(.37, max_height=-.4), M.PLAIN),
    ("max_height NaN", M.world(.37, max_height=np.nan), M.PLAIN),
    ("max_height at the lower bound", M.world(.37, max_height=.02), M.RUNTIME),
    ("max_height below it", M.world(.37, max_height=.0199), M.PLAIN),
    ("max_height at the upper bound", M.world(.37, max_height=2., absorb=1.), M.RUNTIME),
    ("max_height above it", M.world(.37, max_height=2.01, absorb=1.), M.PLAIN),
    ("cld_fuzzy 0", M.world(.37, cld_fuzzy=0.), M.PLAIN),
    ("cld_fuzzy negative", M.world(.37, cld_fuzzy=-.01), M.PLAIN),
    ("cld_fuzzy lost in the sum", M.world(.37, cld_fuzzy=1e-12), M.PLAIN),
    ("coverage above 1", M.world(.37, cld_coverage=1.5), M.RUNTIME),
    ("coverage 0", M.world(.37, cld_coverage=0.), M.RUNTIME),
    ("coverage tiny", M.world(.37, cld_coverage=1e-9), M.PLAIN),
    ("coverage inf", M.world(.37, cld_coverage=np.inf), M.PLAIN),
    ("band edges reversed", M.world(.37, band=(.65, .35, .2)), M.PLAIN),
    ("band edges equal", M.world(.37, band=(.2, .2, .65)), M.PLAIN),
    ("band edge NaN", M.world(.37, band=(.2, np.nan, .65)), M.PLAIN),
    ("band below the ground", M.world(.37, band=(-.5, 0., .65)), M.RUNTIME),
    ("terrain offset 1e6", M.world(.37, terrain_offset=(1e6, 0., 0.)), M.PLAIN),
    ("cloud offset 1e6", M.world(.37, cloud_offset=(0., -1e6, 0.)), M.PLAIN),
    ("offsets at the bound", M.world(.37, terrain_offset=(64., -64., 0.), cloud_offset=(-64., 0., 64.)), M.RUNTIME),
    ("absorb negative", M.world(.37, absorb=-30.), M.RUNTIME),
    ("absorb beyond the exp's domain", M.world(.37, absorb=1e4), M.PLAIN),
    ("absorb beyond it by the step count", M.world(.37, absorb=60., cloud_steps=1), M.PLAIN),
    ("absorb NaN", M.world(.37, absorb=np.nan), M.PLAIN),
    ("cloud_light 0", M.world(.37, cloud_light=0.), M.PLAIN),
    ("cloud_light negative", M.world(.37, cloud_light=-.055), M.RUNTIME),
    ("counts", M.world(.37, terr_steps=512, cloud_steps=256, shadow_steps=32), M.RUNTIME),
] + [(n, M.WORLDS[n], M.RUNTIME) for n in ("recoloured", "overcast", "alpine", "landing")]


@pytest.mark.parametrize("what,Wd,want", TIERS, ids=[t[0] for t in TIERS])
def test_tier_of(what, Wd, want):
    assert M.tier_of(Wd) == want, what
    assert M.tier_of(Wd, variant=1) == M.PLAIN
    assert M.tier_of(Wd, variant=2) == want and M.tier_of(Wd, variant=3) == want
    assert (want == M.RUNTIME) <= M.tame(Wd)
    assert M.refused(Wd) is None


@pytest.mark.parametrize("fn", ["render", "terrain_march", "sdf_terrain_map", "sdf_terrain_map_detail", "sdf_terrain_normal",
                                "clouds_density", "illuminate", "background"])
def test_eval_model_over_the_default_world_is_the_planet_eval_model(fn):
    """sbx_planet_world_eval's definition (evaluate) over default_world(t) against tests/planet_eval_model.py on its families A-E"""
    from tests import planet_eval_model as E
    x = E.inputs(fn)
    for t in (E.TIMES if fn in E.TIME_FNS else (0.0,)):
        assert_same(M.evaluate(M.default_world(t), fn, x), E.evaluate(fn, x, t), (fn, t))


def test_eval_model_render_is_the_frame_before_srgb():
    from tests import planet_eval_model as E
    from tests.model_common import get_primary_ray, point_cam
    Wd = M.WORLDS["landing"]
    fx, fy = np.broadcast_arrays((np.arange(W, dtype=F) + F(.5))[None, :], (np.arange(H, dtype=F) + F(.5))[:, None])
    rd = get_primary_ray(*point_cam(W, H, fx.ravel(), fy.ravel(), F(Wd["fov"])), Wd["eye"], Wd["look_at"])
    rays = np.concatenate([np.tile(np.array(Wd["eye"], dtype=F), (W * H, 1)), np.stack(rd, axis=1)], axis=1)
    lin = M.evaluate(Wd, "render", rays)
    assert_same(E.linear_to_srgb(lin[:, :3]).reshape(H, W, 3), M.fixture("landing")["frame"][..., :3], "landing")


def test_refusals_of_the_model():
    assert M.refused(M.world(terr_steps=0)) == M.refused(M.world(terr_steps=513)) == M.refused(M.world(terr_steps=-1)) == "terr_steps"
    assert M.refused(M.world(cloud_steps=0)) == M.refused(M.world(cloud_steps=257)) == "cloud_steps"
    assert M.refused(M.world(shadow_steps=0)) == M.refused(M.world(shadow_steps=33)) == "shadow_steps"
    assert M.refused(M.world(terr_steps=1, cloud_steps=1, shadow_steps=1)) is None
    assert M.refused(M.world(terr_steps=512, cloud_steps=256, shadow_steps=32)) is None
    assert M.refused(M.world(reserved=(0, 0, 0, 0x80000000))) == "reserved" and M.refused(M.world(reserved=(1, 0, 0, 0))) == "reserved"
