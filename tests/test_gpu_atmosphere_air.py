"""GPU tests of SBX_APP_ATMOSPHERE_AIR (include/sbx.h): src/app_atmosphere.h over the caller's air, bit for bit against
tests/atmosphere_air_model.py and against the frames the reference header itself rendered with the fixture blocks written into it
(tests/golden/atmosphere_airs/): no block = SBX_APP_ATMOSPHERE, the default block of view 1 = SBX_APP_ATMOSPHERE_GROUND; the four
fixtures under the four variants through rows, points, a rank split and the 8-bit format; blocks whose odd values are data into
poisoned buffers, with the tier each launch took (tier_of); alternating blocks; the shared layer checks; host/sbx_render; the refusals."""
import numpy as np
import pytest

from tests import atmosphere_air_model as M
from tests.app_checks import (assert_same, check_multi_render, check_rgba8, check_rows_host_rows_ranks_and_splits, frame_cache, run_sbx_render,
                              same_tensor)
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F

pytestmark = pytest.mark.gpu
APP = "atmosphere_air"
W, H = M.SIZE
W2, H2 = 97, 61
POISON = -7.25
RE = F(6360e3)

BLOCKS = dict(M.AIRS)
ODD = {
    "nan_sun": M.air(.37, sun_dir=(np.nan, .7, -.5)),
    "zero_sun": M.air(.37, sun_dir=(0., 0., 0.)),
    "doubled_sun": M.air(.37, sun_dir=tuple(2 * c for c in M.sun(30., 20.))),
    "sun_below": M.air(.37, sun_dir=M.sun(-20., 75.)),
    "sun_below_runtime": M.air(.37, sun_dir=M.sun(-20., 75.), sun_power=19.),
    "nan_sun_runtime": M.air(.37, sun_dir=(np.nan, .7, -.5), hg_g=.7),
    "shell_inside_out": M.air(.37, atmosphere_radius=6300e3),
    "earth_radius_0": M.air(.37, earth_radius=0.),
    "hR_0": M.air(.37, hR=0.),
    "negative_hM": M.air(.37, hM=-1200.),
    "inf_betaR": M.air(.37, betaR=(5.5e-6, np.inf, 22.4e-6)),
    "negative_betaM": M.air(.37, betaM=(21e-6, -21e-6, 21e-6)),
    "zero_betaR": M.air(.37, betaR=(0., 13e-6, 22.4e-6)),
    "nan_hg_g": M.air(.37, hg_g=np.nan),
    "hg_g_1": M.air(.37, hg_g=1.),
    "eye_at_the_centre": M.air(.37, eye=(0., 0., 0.)),
    "eye_in_space": M.air(.37, eye=(0., 7000e3, 0.), sun_power=25.),
    "fov_0": M.air(.37, fov=0.),
    "counts_1_1": M.air(.37, num_samples=1, num_samples_light=1),
    "counts_64_32": M.air(.37, num_samples=64, num_samples_light=32),
    "view1_from_three_radii": M.air(.37, 1, eye=(0., 3 * RE, 0.), look_at=(0., 0., 0.)),
    "view1_eye_is_look_at": M.air(.37, 1, look_at=(0., RE + F(1.), 0.)),
    "view1_sun_power": M.air(.37, 1, sun_power=19.),
    "view1_doubled_sun": M.air(.37, 1, sun_dir=(0., 2., 0.)),
}
BLOCKS.update(ODD)

model_frame = frame_cache(lambda key, w, h: M.frame(BLOCKS[key], w, h))


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.float32, device=r.tdev)


def moved(before, after, tier):
    """the tier counters after one launch: (launches, literal, plain)"""
    return after == (before[0] + 1, before[1] + (tier == M.LITERAL), before[2] + (tier == M.PLAIN))


@pytest.mark.parametrize("w,h", [(W, H), (W2, H2)])
def test_no_block_and_the_default_blocks_are_the_shipped_apps(renderer, w, h):
    import shaderbox_amd
    for t in (0.0, .37, 2.5):
        sky = renderer.render("atmosphere", w, h, t)
        same_tensor(renderer.render(APP, w, h, t), sky, ("NULL aux", w, h, t))
        before = renderer.atmosphere_air_launches()
        same_tensor(renderer.render(APP, w, h, 99.0, aux=shaderbox_amd.atmosphere_air_default(t)), sky, ("the default block; u_time is not read", w, h, t))
        assert moved(before, renderer.atmosphere_air_launches(), M.LITERAL)
        same_tensor(renderer.render(APP, w, h, 99.0, mouse=(3., 4.), aux=M.as_aux(M.default_air(t))), sky, ("the model's default block", w, h, t))
        ground = renderer.render("atmosphere_ground", w, h, t)
        same_tensor(renderer.render(APP, w, h, 99.0, aux=shaderbox_amd.atmosphere_air_default(t, 1)), ground, ("view 1", w, h, t))
        same_tensor(renderer.render(APP, w, h, 99.0, aux=M.as_aux(M.default_air(t, 1))), ground, ("the model's default block, view 1", w, h, t))
    assert_same(renderer.render(APP, w, h, .37), M.frame(M.default_air(.37), w, h), ("the model", w, h))


@pytest.mark.parametrize("view", [0, 1])
def test_default_blocks_through_the_plain_kernel(renderer, variant_restored, view):
    """sbx_set_variant 1: the air kernel's plain statement over the reference's numbers is the shipped app"""
    import shaderbox_amd
    want = renderer.render("atmosphere_ground" if view else "atmosphere", W2, H2, .37)
    renderer.set_variant(1)
    before = renderer.atmosphere_air_launches()
    same_tensor(renderer.render(APP, W2, H2, 0.0, aux=shaderbox_amd.atmosphere_air_default(.37, view)), want, ("plain", view))
    assert moved(before, renderer.atmosphere_air_launches(), M.PLAIN)


@pytest.mark.parametrize("name", sorted(M.AIRS))
def test_fixture_blocks_are_the_reference(renderer, variant_restored, name):
    import torch
    from shaderbox_amd import shard
    fx, a = M.fixture(name), M.as_aux(M.AIRS[name])
    for variant in (0, 1, 2, 3):
        renderer.set_variant(variant)
        before = renderer.atmosphere_air_launches()
        whole = renderer.render(APP, W, H, 0.0, aux=a)
        assert moved(before, renderer.atmosphere_air_launches(), M.tier_of(M.AIRS[name], variant)), (name, variant)
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


@pytest.mark.parametrize("key", sorted(ODD))
def test_odd_blocks_into_a_poisoned_buffer(renderer, variant_restored, key):
    """97x61: ragged in both directions.  No poison is left and the frame is the model's, whatever it holds; the tier counters move as
    tier_of says"""
    for variant in (0, 1):
        renderer.set_variant(variant)
        before = renderer.atmosphere_air_launches()
        out = renderer.render(APP, W2, H2, 0.0, aux=M.as_aux(ODD[key]), out=poisoned(renderer, W2, H2))
        got = out.cpu().numpy()
        assert not (got == F(POISON)).any(), key
        assert_same(got, model_frame(key, W2, H2), (key, variant))
        assert (got[..., 3] == 1).all()
        assert moved(before, renderer.atmosphere_air_launches(), M.tier_of(ODD[key], variant)), (key, variant)


def test_every_tier_is_among_the_odd_blocks():
    assert {M.tier_of(A) for A in ODD.values()} == {M.LITERAL, M.RUNTIME, M.PLAIN}
    assert M.tier_of(ODD["view1_sun_power"]) == M.RUNTIME and M.tier_of(ODD["eye_in_space"]) == M.RUNTIME


def test_alternating_blocks_keep_their_frames(renderer):
    a, b = M.as_aux(M.AIRS["thin"]), M.as_aux(M.AIRS["aloft"])
    for _ in range(3):
        assert_same(renderer.render(APP, W, H, 0.0, aux=a), M.fixture("thin")["frame"], "thin")
        assert_same(renderer.render(APP, W, H, 0.0, aux=b), M.fixture("aloft")["frame"], "aloft")


def test_shared_layer_checks(renderer):
    """rows, host rows, ranks of 2 and 3, in place, slab pieces: tests/app_checks.py, as for any app"""
    check_rows_host_rows_ranks_and_splits(renderer, APP, W, H, 0.0, M.fixture("aloft")["frame"], cuts=(7, 20), aux=M.as_aux(M.AIRS["aloft"]))


def test_main_image_and_batch(renderer):
    fx, a = M.fixture("coarse"), M.as_aux(M.AIRS["coarse"])
    got = renderer.main_image_batch(APP, W, H, 0.0, fx["points"], aux=a)
    assert_same(got, fx["points_out"], "main_image_batch")
    one = renderer.main_image(APP, W, H, 0.0, tuple(float(v) for v in fx["points"][3]), aux=a)
    assert_same(np.asarray(one, dtype=F).reshape(4), fx["points_out"][3], "main_image")


def test_multi_render():
    check_multi_render(APP, W, H, .37, lambda: M.frame(M.default_air(.37), W, H))


def test_sbx_render_app_atmosphere_air(tmp_path):
    """host/sbx_render --app atmosphere_air with one flag per field: the `thin` and `aloft` fixtures (the block starts as the default of
    --time and --air-view); without flags: SBX_APP_ATMOSPHERE's frame of --time"""
    c = lambda v: ",".join(repr(float(x)) for x in v)  # noqa: E731
    s = lambda v: repr(float(v))  # noqa: E731
    A = M.AIRS["thin"]
    flags = ("--air-earth-radius", s(A["earth_radius"]), "--air-atmosphere-radius", s(A["atmosphere_radius"]), "--air-h-r", s(A["hR"]), "--air-h-m", s(A["hM"]),
             "--air-beta-r", c(A["betaR"]), "--air-beta-m", c(A["betaM"]), "--air-sun-power", s(A["sun_power"]), "--air-sun", c(A["sun_dir"]),
             "--air-eye", c(A["eye"]))
    assert_same(run_sbx_render(tmp_path, APP, W, H, .37, flags=flags), M.fixture("thin")["frame"], "--app atmosphere_air, thin")
    A = M.AIRS["aloft"]
    flags = ("--air-view", "1", "--air-eye", c(A["eye"]), "--air-look-at", c(A["look_at"]), "--air-fov", s(A["fov"]), "--air-hg-g", s(A["hg_g"]),
             "--air-sun-power", s(A["sun_power"]), "--air-sun", c(A["sun_dir"]), "--air-samples", "16", "--air-samples-light", "8")
    assert_same(run_sbx_render(tmp_path, APP, W, H, 0.0, flags=flags), M.fixture("aloft")["frame"], "--app atmosphere_air, aloft")
    assert_same(run_sbx_render(tmp_path, APP, W, H, 2.5), M.frame(M.default_air(2.5), W, H), "--app atmosphere_air, no flags")


REFUSED = {"view_2": M.air(view=2), "view_minus_1": M.air(view=-1), "no_samples": M.air(num_samples=0), "samples_65": M.air(num_samples=65),
           "no_light_samples": M.air(num_samples_light=0), "light_samples_33": M.air(num_samples_light=33), "reserved0": M.air(reserved0=7),
           "reserved_word": M.air(reserved=(0., 0., 0., 0., 0., 1.)), "reserved_minus_zero": M.air(reserved=(-0., 0., 0., 0., 0., 0.))}


@pytest.mark.parametrize("key", sorted(REFUSED))
def test_refusals_leave_the_buffer_alone(renderer, key):
    import shaderbox_amd
    import torch
    assert M.refused(REFUSED[key]) is not None
    before = renderer.atmosphere_air_launches()
    out = poisoned(renderer, W, H)
    with pytest.raises(shaderbox_amd.SbxError) as e:
        renderer.render(APP, W, H, 0.0, aux=M.as_aux(REFUSED[key]), out=out)
    assert e.value.code == shaderbox_amd.SBX_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == POISON).all()), key
    assert renderer.atmosphere_air_launches() == before
