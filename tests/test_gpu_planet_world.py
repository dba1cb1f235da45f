"""GPU tests of SBX_APP_PLANET_WORLD (include/sbx.h): src/app_planet.h as shipped over the caller's world, bit for bit
against tests/planet_world_model.py and against the frames the reference header itself rendered with the fixture worlds written into
it (tests/golden/planet_worlds/): no block = SBX_APP_PLANET; the five fixtures under the four kernel variants through rows, points, a
rank split and the 8-bit format; odd blocks (a NaN sun, an inf spin, eye == look_at, max_height 0 and negative, cld_fuzzy 0, reversed
band edges, coverage above 1, offsets of 1e6, fov 0, a huge eye) into poisoned buffers with the launch record showing what each ran;
alternating worlds; ten launches of one world; the shared layer checks; the refusals."""
import numpy as np
import pytest

from tests import planet_world_model as M
from tests.app_checks import (assert_same, check_multi_render, check_rgba8, check_rows_host_rows_ranks_and_splits, frame_cache, same_tensor)
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F

pytestmark = pytest.mark.gpu
APP = "planet_world"
W, H = M.SIZE
W2, H2 = 97, 61
POISON = -7.25
TIER_INDEX = {M.LITERAL: 0, M.RUNTIME: 1, M.PLAIN: 2}

WORLDS = dict(M.WORLDS)
COLOUR = dict(c_rock=(.1, .05, .03))                  # one number restated: the run-time kernel's business
ODD = {
    "nan_sun": M.world(.37, sun_dir=(np.nan, .7, -.5)),
    "nan_sun_runtime": M.world(.37, sun_dir=(np.nan, .7, -.5), **COLOUR),
    "zero_sun": M.world(.37, sun_dir=(0., 0., 0.), **COLOUR),
    "inf_spin": M.world(.37, spin_deg=np.inf),
    "inf_spin_runtime": M.world(.37, spin_deg=np.inf, **COLOUR),
    "eye_is_look_at": M.world(.37, eye=(0., 0., 2.)),
    "eye_is_look_at_runtime": M.world(.37, eye=(0., 0., 2.), **COLOUR),
    "max_height_0": M.world(.37, max_height=0.),
    "max_height_negative": M.world(.37, max_height=-.4),
    "cld_fuzzy_0": M.world(.37, cld_fuzzy=0.),
    "band_reversed": M.world(.37, band=(.65, .35, .2)),
    "coverage_above_1": M.world(.37, cld_coverage=1.5),
    "terrain_offset_1e6": M.world(.37, terrain_offset=(1e6, -1e6, 1e6)),
    "cloud_offset_1e6": M.world(.37, cloud_offset=(1e6, 1e6, -1e6)),
    "fov_0": M.world(.37, fov=0.),
    "fov_0_runtime": M.world(.37, fov=0., **COLOUR),
    "huge_eye": M.world(.37, eye=(0., 0., -3e30)),
    "huge_eye_runtime": M.world(.37, eye=(0., 0., -3e30), **COLOUR),
    "far_eye_runtime": M.world(.37, eye=(0., 0., -2e4), **COLOUR),      # finite rays whose hit_o leaves the sphere: the wave's test
    "eye_inside_the_planet": M.world(.37, eye=(.1, .2, -.3), **COLOUR),
    "negative_cloud_light": M.world(.37, cloud_light=-.055),
    "one_step_each": M.world(.37, terr_steps=1, cloud_steps=1, shadow_steps=1),
    "most_steps": M.world(.37, terr_steps=512, cloud_steps=256, shadow_steps=32),
}
WORLDS.update(ODD)

model_frame = frame_cache(lambda key, w, h: M.frame(WORLDS[key], w, h))


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.float32, device=r.tdev)


@pytest.mark.parametrize("w,h", [(W, H), (W2, H2)])
def test_no_block_is_the_shipped_app(renderer, w, h):
    import shaderbox_amd
    for t in (0.0, .37, 2.5):
        planet = renderer.render("planet", w, h, t)
        same_tensor(renderer.render(APP, w, h, t), planet, ("NULL aux", w, h, t))
        same_tensor(renderer.render(APP, w, h, 99.0, aux=shaderbox_amd.planet_world_default(t)), planet, ("the default block; u_time is not read", w, h, t))
        same_tensor(renderer.render(APP, w, h, 99.0, mouse=(3., 4.), aux=M.as_aux(M.default_world(t))), planet, ("the model's default block", w, h, t))
    assert_same(renderer.render(APP, w, h, .37), M.frame(M.default_world(.37), w, h), ("the model", w, h))


@pytest.mark.parametrize("name", sorted(M.WORLDS))
def test_fixture_worlds_are_the_reference(renderer, variant_restored, name):
    import torch
    from shaderbox_amd import shard
    fx, a = M.fixture(name), M.as_aux(M.WORLDS[name])
    for variant in (0, 1, 2, 3):
        renderer.set_variant(variant)
        before = renderer.planet_world_launches()
        whole = renderer.render(APP, W, H, 0.0, aux=a)
        after = renderer.planet_world_launches()
        want = [0, 0, 0]
        want[TIER_INDEX[M.tier_of(M.WORLDS[name], variant)]] = 1
        assert [y - x for x, y in zip(before, after)] == want, (name, variant, before, after)
        assert_same(whole, fx["frame"], (name, "frame", variant))
        parts = [renderer.render(APP, W, H, 0.0, aux=a, rows=(r0, r1)) for r0, r1 in ((0, 5), (5, 24), (24, H))]
        same_tensor(torch.cat(parts), whole, (name, "rows", variant))
        assert_same(renderer.render_points(APP, W, H, 0.0, torch.from_numpy(fx["points"]), aux=a), fx["points_out"], (name, "points", variant))
        assert_same(renderer.render(APP, W2, H2, 0.0, aux=a), model_frame(name, W2, H2), (name, "97x61", variant))
    renderer.set_variant(0)
    n, br = 2, 8                                                      # one rank split, gathered and assembled
    rows_max = shard.rank_rows_max(H, br, n, 1, 1)
    gathered = torch.empty((n * rows_max, W, 4), dtype=torch.float32, device=renderer.tdev)
    for r in range(n):
        renderer.render_rank(APP, W, H, 0.0, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], aux=a, root_rounds=1, rounds=1)
    assert_same(renderer.assemble(gathered, W, H, br, n, root_rounds=1, rounds=1), fx["frame"], (name, "rank split"))
    assert_same(check_rgba8(renderer, APP, W, H, 0.0, aux=a), fx["frame"], (name, "the float frame beside the 8-bit one"))


def test_default_world_with_one_colour_bit_changed_takes_the_runtime_kernel(renderer):
    """the same work as SBX_APP_PLANET through the other kernel: a snow one ulp brighter changes the pixels it colours and no others"""
    Wd = M.world(.37, c_snow=(np.nextafter(F(.6), F(1)), .6, .6))
    before = renderer.planet_world_launches()
    got = renderer.render(APP, W2, H2, 0.0, aux=M.as_aux(Wd)).cpu().numpy()
    after = renderer.planet_world_launches()
    assert [y - x for x, y in zip(before, after)] == [0, 1, 0]
    assert_same(got, M.frame(Wd, W2, H2), "one colour bit")
    planet = renderer.render("planet", W2, H2, .37).cpu().numpy()
    changed = M.differing(got, planet)
    assert 0 < changed.sum() < .2 * W2 * H2, int(changed.sum())


@pytest.mark.parametrize("key", sorted(ODD))
def test_odd_worlds_into_a_poisoned_buffer(renderer, variant_restored, key):
    """97x61: ragged in both directions.  No poison is left and the frame is the model's, whatever it holds; the launch record shows
    the tier the model's tier_of names, under the default variant and under 3"""
    for variant in (0, 3):
        renderer.set_variant(variant)
        before = renderer.planet_world_launches()
        out = renderer.render(APP, W2, H2, 0.0, aux=M.as_aux(ODD[key]), out=poisoned(renderer, W2, H2))
        got = out.cpu().numpy()
        after = renderer.planet_world_launches()
        assert not (got == F(POISON)).any(), key
        assert_same(got, model_frame(key, W2, H2), (key, variant))
        assert (got[..., 3] == 1).all()
        want = [0, 0, 0]
        want[TIER_INDEX[M.tier_of(ODD[key], variant)]] = 1
        assert [y - x for x, y in zip(before, after)] == want, (key, variant, before, after)


def test_edge_points_under_a_tame_world(renderer, variant_restored):
    """fragCoords far outside the frame, at 1e30, inf and NaN (app_checks.edge_points) under a run-time world: the waves whose rays
    leave the wave-wide test's set take the plain body, and both kernels give the same bits"""
    import torch
    from tests.app_checks import edge_points
    pts = torch.from_numpy(edge_points(W, H))
    a = M.as_aux(M.WORLDS["alpine"])
    renderer.set_variant(0)
    fast = renderer.render_points(APP, W, H, 0.0, pts, aux=a).cpu().numpy()
    renderer.set_variant(1)
    plain = renderer.render_points(APP, W, H, 0.0, pts, aux=a).cpu().numpy()
    assert_same(fast, plain, "edge points, run-time against plain")
    some = np.arange(0, 400, 7)                                        # the model on a sample of the in-frame ones
    assert_same(fast[some], M.points(M.WORLDS["alpine"], W, H, pts.numpy()[some]), "edge points against the model")


def test_alternating_worlds_keep_their_frames(renderer):
    a, b, c = (M.as_aux(M.WORLDS[n]) for n in ("overcast", "orbit", "landing"))
    for _ in range(3):
        assert_same(renderer.render(APP, W, H, 0.0, aux=a), M.fixture("overcast")["frame"], "overcast")
        assert_same(renderer.render(APP, W, H, 0.0, aux=b), M.fixture("orbit")["frame"], "orbit")
        assert_same(renderer.render(APP, W, H, 0.0, aux=c), M.fixture("landing")["frame"], "landing")


def test_a_world_that_stands_still_keeps_its_bits(renderer):
    """500x515: ragged tiles.  Ten launches of one world into poisoned buffers, then another world"""
    import torch
    from tests.app_checks import bits_differ
    w, h = 500, 515
    a = M.as_aux(M.WORLDS["alpine"])
    first = None
    for k in range(10):
        got = renderer.render(APP, w, h, 0.0, aux=a, out=poisoned(renderer, w, h))
        torch.cuda.synchronize()
        if first is None:
            first = got.clone()
            assert not bool((first == POISON).any())
        assert bits_differ(got, first) == 0, ("launch", k + 1)
    assert_same(renderer.render(APP, W, H, 0.0, aux=M.as_aux(M.WORLDS["recoloured"])), M.fixture("recoloured")["frame"], "recoloured after alpine's launches")


def test_shared_layer_checks(renderer):
    """rows, host rows, ranks of 2 and 3, in place, slab pieces: tests/app_checks.py, as for any app"""
    check_rows_host_rows_ranks_and_splits(renderer, APP, W, H, 0.0, M.fixture("overcast")["frame"], cuts=(7, 20), aux=M.as_aux(M.WORLDS["overcast"]))


def test_main_image_and_batch(renderer):
    fx, a = M.fixture("landing"), M.as_aux(M.WORLDS["landing"])
    got = renderer.main_image_batch(APP, W, H, 0.0, fx["points"], aux=a)
    assert_same(got, fx["points_out"], "main_image_batch")
    one = renderer.main_image(APP, W, H, 0.0, tuple(float(v) for v in fx["points"][3]), aux=a)
    assert_same(np.asarray(one, dtype=F).reshape(4), fx["points_out"][3], "main_image")


def test_multi_render():
    check_multi_render(APP, W, H, .37, lambda: M.frame(M.default_world(.37), W, H))


def world_flags(Wd, t):
    """one --world-<field> flag per field of Wd that differs from the default world of u_time t"""
    D, flags = M.default_world(t), []
    for k in M.FIELDS:
        if k == "reserved" or np.array_equal(np.asarray(Wd[k]), np.asarray(D[k])):
            continue
        v = Wd[k]
        flags += ["--world-" + k.replace("_", "-"), str(v) if k in M.INT_FIELDS else ",".join(repr(float(x)) for x in v) if isinstance(v, tuple) else repr(float(v))]
    return flags


def test_sbx_render_app_planet_world(tmp_path):
    """host/sbx_render --app planet_world with one flag per field: the `overcast` and `landing` fixtures (the block starts as the world
    of --time); without flags: SBX_APP_PLANET's frame of --time"""
    from tests.app_checks import run_sbx_render
    for name in ("overcast", "landing"):
        flags = world_flags(M.WORLDS[name], M.T0)
        assert len(flags) >= 10, name                                  # five fields or more each
        assert_same(run_sbx_render(tmp_path, APP, W, H, M.T0, flags=flags), M.fixture(name)["frame"], "--app planet_world, " + name)
    assert_same(run_sbx_render(tmp_path, APP, W, H, 2.5), M.frame(M.default_world(2.5), W, H), "--app planet_world, no flags")


def test_refusals_write_nothing(renderer):
    import shaderbox_amd
    bad = [M.world(terr_steps=0), M.world(terr_steps=513), M.world(cloud_steps=0), M.world(cloud_steps=257), M.world(shadow_steps=0),
           M.world(shadow_steps=33), M.world(reserved=(0, 0, 1, 0)), M.world(reserved=(0x80000000, 0, 0, 0))]
    for Wd in bad:
        assert M.refused(Wd) is not None
        out = poisoned(renderer, W, H)
        before = renderer.planet_world_launches()
        with pytest.raises(shaderbox_amd.SbxError) as e:
            renderer.render(APP, W, H, 0.0, aux=M.as_aux(Wd), out=out)
        assert e.value.code == shaderbox_amd.SBX_ERR_ARG, M.refused(Wd)
        assert bool((out == POISON).all()) and renderer.planet_world_launches() == before
    assert_same(renderer.render(APP, W, H, 0.0, aux=M.as_aux(M.WORLDS["alpine"])), M.fixture("alpine")["frame"], "the context renders on")
