"""GPU tests of SBX_APP_VINYL_DECK (include/sbx.h): src/app_vinyl.h as shipped over the caller's deck, bit for bit against
tests/vinyl_deck_model.py and against the frames the reference header itself rendered with the fixture decks written into it
(tests/golden/vinyl_decks/): no block = SBX_APP_VINYL; the four fixtures under the four kernel variants through rows, points, a rank
split and the 8-bit format; decks outside the domain of k_vinyl's culls (a far eye, a NaN sun, eye == look_at, non-finite angles) into
poisoned buffers, and the record that they took the plain kernel; decks whose odd values are data (a zero sun, a sun below the disc,
a_x = 0, a negative colour); alternating decks; the shared layer checks; host/sbx_render."""
import numpy as np
import pytest

from tests import vinyl_deck_model as M
from tests.app_checks import (assert_same, check_multi_render, check_rgba8, check_rows_host_rows_ranks_and_splits, frame_cache, run_sbx_render,
                              same_tensor)
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F

pytestmark = pytest.mark.gpu
APP = "vinyl_deck"
W, H = M.SIZE
W2, H2 = 97, 61
POISON = -7.25

DECKS = dict(M.DECKS)
DECKS["nan_sun"] = M.deck(.37, sun_dir=(np.nan, .7, -.5))
DECKS["eye_is_look_at"] = M.deck(.37, eye=(0., 5.75, 6.75), look_at=(0., 5.75, 6.75))
DECKS["inf_platter"] = M.deck(.37, platter_deg=np.inf)
DECKS["nan_arm_tilt"] = M.deck(.37, arm_tilt_deg=np.nan)
DECKS["huge_sun"] = M.deck(.37, sun_dir=(-1e5, 4e5, -3e5))
UNTAME = ("far", "nan_sun", "eye_is_look_at", "inf_platter", "nan_arm_tilt", "huge_sun")
DECKS["zero_sun"] = M.deck(.37, sun_dir=(0., 0., 0.))
DECKS["sun_below"] = M.deck(.37, sun_dir=(.3, -.8, .2))
DECKS["a_x_zero"] = M.deck(.37, a_x=0.)
DECKS["negative_colour"] = M.deck(.37, groove_color=(-.01, .02, -.5), shiny_color=(-1., -1., .5), shininess=-2.)
DECKS["fov0"] = M.deck(.37, fov=0.)
TAME_ODD = ("zero_sun", "sun_below", "a_x_zero", "negative_colour", "fov0")

model_frame = frame_cache(lambda key, w, h: M.frame(M.scene_of(DECKS[key]), w, h))


def poisoned(r, w, h):
    import torch
    return torch.full((h, w, 4), POISON, dtype=torch.float32, device=r.tdev)


@pytest.mark.parametrize("w,h", [(W, H), (W2, H2)])
def test_no_block_is_the_shipped_app(renderer, w, h):
    import shaderbox_amd
    for t in (0.0, .37, 2.5):
        vinyl = renderer.render("vinyl", w, h, t)
        same_tensor(renderer.render(APP, w, h, t), vinyl, ("NULL aux", w, h, t))
        same_tensor(renderer.render(APP, w, h, 99.0, aux=shaderbox_amd.vinyl_deck_default(t)), vinyl, ("the default block; u_time is not read", w, h, t))
        same_tensor(renderer.render(APP, w, h, 99.0, mouse=(3., 4.), aux=M.as_aux(M.default_deck(t))), vinyl, ("the model's default block", w, h, t))
    assert_same(renderer.render(APP, w, h, .37), M.frame(M.scene_of(M.default_deck(.37)), w, h), ("the model", w, h))


@pytest.mark.parametrize("name", sorted(M.DECKS))
def test_fixture_decks_are_the_reference(renderer, variant_restored, name):
    import torch
    from shaderbox_amd import shard
    fx, a = M.fixture(name), M.as_aux(M.DECKS[name])
    for variant in (0, 1, 2, 3):
        renderer.set_variant(variant)
        whole = renderer.render(APP, W, H, 0.0, aux=a)
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


@pytest.mark.parametrize("key", UNTAME + TAME_ODD)
def test_odd_decks_into_a_poisoned_buffer(renderer, variant_restored, key):
    """97x61: ragged in both directions.  No poison is left and the frame is the model's, whatever it holds; a deck outside the culls'
    domain is recorded as a launch of the plain kernel whatever variant is set, a tame one never is"""
    for variant in (0, 3):
        renderer.set_variant(variant)
        launches, untame = renderer.vinyl_deck_launches()
        out = renderer.render(APP, W2, H2, 0.0, aux=M.as_aux(DECKS[key]), out=poisoned(renderer, W2, H2))
        got = out.cpu().numpy()
        assert not (got == F(POISON)).any(), key
        assert_same(got, model_frame(key, W2, H2), (key, variant))
        assert (got[..., 3] == 1).all()
        after = renderer.vinyl_deck_launches()
        assert after == (launches + 1, untame + (1 if key in UNTAME else 0)), (key, variant, after)


def test_alternating_decks_keep_their_frames(renderer):
    """one deck after another on one context: the block is part of the dispatch-order table's key, neither is served the other's"""
    a, b = M.as_aux(M.DECKS["scratch"]), M.as_aux(M.DECKS["dusk"])
    for _ in range(4):
        assert_same(renderer.render(APP, W, H, 0.0, aux=a), M.fixture("scratch")["frame"], "scratch")
        assert_same(renderer.render(APP, W, H, 0.0, aux=b), M.fixture("dusk")["frame"], "dusk")


def test_a_deck_that_stands_still_keeps_its_bits_under_a_table(renderer):
    """500x515: ragged tiles.  Ten launches of one deck into poisoned buffers (a tile a table lost would stay poison), then another deck"""
    import torch
    from tests.app_checks import bits_differ
    w, h = 500, 515
    a = M.as_aux(M.DECKS["scratch"])
    first = None
    for k in range(10):
        got = renderer.render(APP, w, h, 0.0, aux=a, out=poisoned(renderer, w, h))
        torch.cuda.synchronize()
        if first is None:
            first = got.clone()
            assert not bool((first == POISON).any())
        assert bits_differ(got, first) == 0, ("launch", k + 1)
    assert_same(renderer.render(APP, W, H, 0.0, aux=M.as_aux(M.DECKS["coloured"])), M.fixture("coloured")["frame"], "coloured after scratch's launches")


def test_shared_layer_checks(renderer):
    """rows, host rows, ranks of 2 and 3, in place, slab pieces: tests/app_checks.py, as for any app"""
    check_rows_host_rows_ranks_and_splits(renderer, APP, W, H, 0.0, M.fixture("coloured")["frame"], cuts=(7, 20), aux=M.as_aux(M.DECKS["coloured"]))


def test_main_image_and_batch(renderer):
    fx, a = M.fixture("dusk"), M.as_aux(M.DECKS["dusk"])
    got = renderer.main_image_batch(APP, W, H, 0.0, fx["points"], aux=a)
    assert_same(got, fx["points_out"], "main_image_batch")
    one = renderer.main_image(APP, W, H, 0.0, tuple(float(v) for v in fx["points"][3]), aux=a)
    assert_same(np.asarray(one, dtype=F).reshape(4), fx["points_out"][3], "main_image")


def test_multi_render():
    check_multi_render(APP, W, H, .37, lambda: M.frame(M.scene_of(M.default_deck(.37)), W, H))


def test_sbx_render_app_vinyl_deck(tmp_path):
    """host/sbx_render --app vinyl_deck with one flag per field: the `coloured` and `scratch` fixtures (the block starts as the deck of
    --time); without flags: SBX_APP_VINYL's frame of --time"""
    c = lambda v: ",".join(repr(float(x)) for x in v)  # noqa: E731
    D = M.DECKS["coloured"]
    flags = ("--groove-color", c(D["groove_color"]), "--dead-wax-color", c(D["dead_wax_color"]), "--label-color", c(D["label_color"]),
             "--logo-color", c(D["logo_color"]), "--shiny-color", c(D["shiny_color"]), "--ro-spec", repr(float(D["ro_spec"])),
             "--a-x", repr(float(D["a_x"])), "--a-y", repr(float(D["a_y"])), "--shininess", repr(float(D["shininess"])))
    assert_same(run_sbx_render(tmp_path, APP, W, H, .37, flags=flags), M.fixture("coloured")["frame"], "--app vinyl_deck, coloured")
    D = M.DECKS["scratch"]
    flags = ("--platter-deg", repr(float(D["platter_deg"])), "--platter-tilt", repr(float(D["platter_tilt_deg"])), "--arm-tilt", repr(float(D["arm_tilt_deg"])),
             "--deck-eye", c(D["eye"]), "--deck-look-at", c(D["look_at"]), "--deck-fov", repr(float(D["fov"])), "--deck-sun", c(D["sun_dir"]))
    assert_same(run_sbx_render(tmp_path, APP, W, H, 0.0, flags=flags), M.fixture("scratch")["frame"], "--app vinyl_deck, scratch")
    assert_same(run_sbx_render(tmp_path, APP, W, H, 2.5), M.frame(M.scene_of(M.default_deck(2.5)), W, H), "--app vinyl_deck, no flags")
