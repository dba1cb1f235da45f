"""CPU tests of the definition of SBX_APP_VINYL_DECK and sbx_vinyl_eval (include/sbx.h): tests/vinyl_deck_model.py against
the oracle (the shipped deck), against the close-up build's fixture with that camera in the block, and against the frames and points the
reference header itself rendered with the four fixture decks written into it (tests/golden/vinyl_decks/,
tools/make_golden_vinyl_decks.py); the conditions on those fixtures; the single-field property; the block sbx_vinyl_deck_default
returns; "render" tied to the frame."""
import ctypes
import os

import numpy as np
import pytest

from tests import vinyl_builds_model as V
from tests import vinyl_deck_model as M
from tests.app_checks import assert_same, frame_cache

F = np.float32
W, H = M.SIZE

shares_of = frame_cache(lambda name: M.shares(M.scene_of(M.DECKS[name]), W, H))
default_of = frame_cache(lambda: M.shares(M.scene_of(M.default_deck(0.)), W, H))


@pytest.mark.parametrize("w,h", [(64, 64), (64, 36)])
def test_default_deck_equals_the_oracle(oracle, w, h):
    from oracle.oracle import APP_IDS
    for t in (0.0, .37, 2.5):
        got = M.frame(M.scene_of(M.default_deck(t)), w, h)
        assert (got[..., 3] == 1).all()
        assert_same(got, oracle.render(APP_IDS["vinyl"], w, h, t), ("default deck", w, h, t))


def test_closeup_camera_in_the_block_equals_the_closeup_builds_fixture():
    """tests/golden/vinyl_builds/: what the reference header rendered with setup_camera's `#else` pair"""
    eye, look_at = V.CAMERA["closeup"]
    fx = V.fixture("closeup")
    assert len(fx["frames"]) >= 1
    for u, frame in zip(fx["uniforms"], fx["frames"]):
        w, h, t = int(u[0]), int(u[1]), u[4]
        assert_same(M.frame(M.scene_of(M.deck(t, eye=eye, look_at=look_at)), w, h), frame, ("closeup", w, h, t))


def test_block_layout_and_the_librarys_default():
    """sbx_vinyl_deck_default (host code, no GPU): the model's default_deck in every bit; the block is 128 bytes"""
    import shaderbox_amd
    assert ctypes.sizeof(shaderbox_amd.VinylDeck) == 128 and [n for n, _ in shaderbox_amd.VinylDeck._fields_] == list(M.FIELDS)
    for t in (0.0, .37, 2.5, -0.41, 1e9, float("nan")):
        a = shaderbox_amd.vinyl_deck_default(t)
        want = M.default_deck(t)
        for name in M.FIELDS:                        # field by field
            got = getattr(a, name)
            got = np.array(list(got) if hasattr(got, "__len__") else [got], dtype=F)
            assert_same(got, np.array(want[name], dtype=F).reshape(-1), ("sbx_vinyl_deck_default", t, name))
        assert_same(np.frombuffer(bytes(a), dtype=F), M.block(want), ("sbx_vinyl_deck_default", t))
    D = M.DECKS["coloured"]
    b = shaderbox_amd.vinyl_deck(.37, **{k: (list(map(float, D[k])) if isinstance(D[k], tuple) else float(D[k])) for k in
                                         ("groove_color", "dead_wax_color", "label_color", "logo_color", "shiny_color", "ro_spec", "a_x", "a_y", "shininess")})
    assert_same(np.frombuffer(bytes(b), dtype=F), M.block(D), "vinyl_deck")


@pytest.mark.parametrize("name", sorted(M.DECKS))
def test_model_equals_the_reference_fixture(name):
    z = M.fixture(name)
    assert set(z.files) == {"deck", "frame", "points", "points_out"}
    assert_same(z["deck"], M.block(M.DECKS[name]), (name, "deck"))
    assert z["frame"].shape == (H, W, 4) and z["points"].shape == (M.POINTS, 2) and z["points_out"].shape == (M.POINTS, 4)
    assert_same(z["points"], M.fixture_points(M.POINT_SEEDS[name], W, H, M.POINTS), (name, "points"))
    assert_same(shares_of(name)[1], z["frame"], (name, "frame"))
    assert_same(M.points(M.scene_of(M.DECKS[name]), W, H, z["points"]), z["points_out"], (name, "points_out"))
    root = os.path.dirname(M.GOLDEN)
    bound = max(os.path.getsize(os.path.join(M.GOLDEN, f)) for f in os.listdir(M.GOLDEN) if f.endswith(".npz"))
    assert os.path.getsize(os.path.join(M.GOLDEN, "vinyl_decks", "%s_%dx%d.npz" % (name, W, H))) <= bound, root


def test_fixture_conditions():
    for name in M.DECKS:
        print(name, {k: (round(float(v), 4) if k != "logo_pixels" else v) for k, v in shares_of(name)[0].items() if k not in ("hit", "mat")})
    M.check_conditions({n: shares_of(n)[0] for n in M.DECKS}, {n: M.fixture(n)["frame"] for n in M.DECKS}, *default_of())


@pytest.mark.parametrize("field", sorted(M.READERS))
def test_one_field_alone_changes_the_pixels_that_read_it(field):
    """model against model over the 64x36 frame: at least one pixel changes, and none whose material does not read the field"""
    base_s, base = default_of()
    changed = M.differing(M.frame(M.scene_of(M.single_field_decks()[field]), W, H), base)
    assert changed.any(), field
    if M.READERS[field] is not None:
        assert not (changed & ~np.isin(base_s["mat"], M.READERS[field])).any(), field


def test_rays_of_a_frame_tie_render_to_the_pixel():
    """render over the primary rays, then sRGB: the frame; t and the material id beside it"""
    D = M.DECKS["scratch"]
    fx, fy = M.frame_coords(W, H)
    ro, rd = M.primary_rays(D, W, H, fx, fy)
    rgb, t, mat = M.render(M.scene_of(D), ro, rd)
    assert_same(M.finish(rgb).reshape(H, W, 4), M.fixture("scratch")["frame"], "render + finish")
    assert ((mat > 0) == (rgb != 1).any(axis=1) | (mat > 0)).all() and set(np.unique(mat)) == {0., 1., 2., 3., 4., 5.}
    assert (t[mat == 0] > 40).all() or (t[mat == 0] > 0).all()


def test_material_ids_outside_the_table():
    """int() toward zero, saturating, NaN -> 0; an id outside 1-5 takes the else branch, white for 0 and the zero colour for any other"""
    assert list(M.to_int(np.array([2.9, -.5, np.nan, 1e20, -1e20, 5., -3.2], dtype=F))) == [2, 0, 0, 2147483520, -2147483648, 5, -3]
    S = M.scene_of(M.default_deck(0.))
    eye, p = (F(0), F(5), F(0)), (np.full(3, F(2.5)), np.full(3, F(.05)), np.zeros(3, dtype=F))
    lit = M.illuminate(S, eye, p, np.array([0, 7, -1], dtype=np.int32))
    assert (lit[0] > lit[1]).all() and same_rows(lit[1], lit[2])


def same_rows(a, b):
    return bool(M.same_bits(a, b).all())
