"""CPU tests of sbx_sdf_scene_eval's definition (tests/sdf_scene_eval_model.py; include/sbx.h): `render` over the
primary rays of every fixture scene is, after the app's sRGB step, the scene model's frame and the frame the reference's own headers
rendered; `sdf` is the scene model's; the restated sdf_shadow is the scene model's for a constant direction; `render_impl` is the chain
of the other functions at its own hit points; the Python binding states the entry's widths; and the element families of
tests/sdf_scene_eval_cases.py meet the conditions under which the GPU tests say something."""
import numpy as np
import pytest

from tests import sdf_scene_eval_cases as C
from tests import sdf_scene_eval_model as E
from tests import sdf_scene_model as M
from tests.model_common import F, same_bits

W, H = C.SIZE


def differing(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((~same_bits(a, b)).reshape(len(a), -1).any(axis=-1).sum())


def test_widths_are_the_bindings():
    from shaderbox_amd import Renderer
    assert Renderer.EVAL_WIDTHS["sdf_scene"] == {"sdf": (3, 2), "sdf_normal": (3, 3), "sdf_ao": (6, 1), "sdf_shadow": (6, 1),
                                                 "illuminate": (9, 3), "render_impl": (6, 5), "render": (6, 4)}
    assert Renderer.EVAL_WIDTHS["sdf_scene"] == E.WIDTHS and tuple(Renderer.EVAL_WIDTHS["sdf_scene"]) == E.FNS, "in name-list order"
    assert callable(Renderer.sdf_scene_eval) and callable(Renderer.sdf_scene_eval_counted)


@pytest.mark.parametrize("name", list(M.scenes()))
def test_render_over_the_primary_rays_is_the_references_frame(name):
    assert tuple(M.scene_table()["size"]) == C.SIZE
    S = M.scenes()[name]
    out = E.evaluate("render", S, E.primary_rays(S, W, H))
    got = E.finish(out[:, :3]).reshape(H, W, 4)
    assert differing(got, M.frame(S, W, H)) == 0, name
    assert differing(got, M.fixture(name)["frame"]) == 0, (name, "fixture")
    impl = E.evaluate("render_impl", S, E.primary_rays(S, W, H))
    assert same_bits(impl[:, 3], out[:, 3]).all(), "orig.w is render_impl's t"
    masks = M.masks(S, W, H)
    assert np.array_equal(impl[:, 4] >= 0, masks["hit"]) and set(impl[:, 4].tolist()) <= {-1., 0., 1., 2., 3., 4., 5., 6., 7.}


def test_sdf_is_the_scene_models():
    for name in ("seeded", "centres", "specials", "frame_plain"):
        S, x = C.scene_of(name), C.family(name, "sdf")
        d, m = M.sdf(S, x[:, 0], x[:, 1], x[:, 2])
        assert differing(E.evaluate("sdf", S, x), np.stack([d, m], axis=1).astype(F)) == 0, name


def test_the_restated_shadow_is_the_scene_models_for_one_direction():
    for name in ("frame_shadow", "frame_short", "centres"):
        S = C.scene_of(name)
        sun = tuple(F(v) for v in S["sun_dir"])
        o = C.family(name, "sdf_shadow")[:, :3]
        x = np.concatenate([o, np.broadcast_to(np.asarray(sun, dtype=F), o.shape)], axis=1).astype(F)
        a, b = {}, {}
        want = M.sdf_shadow(M.scene_sdf(S), sun, o[:, 0], o[:, 1], o[:, 2], a)
        assert differing(E.evaluate("sdf_shadow", S, x, b), want[:, None]) == 0, name
        assert np.array_equal(a["exit"], b["exit"])


@pytest.mark.parametrize("name", [n for n in C.FAMILIES if n != "specials"])
def test_render_impl_is_the_chain_at_its_own_hit_points(name):
    """sdf_normal -> sdf_ao -> sdf_shadow(p + sun * .05, sun) under the block's switch -> illuminate, each through evaluate()"""
    S, rays = C.scene_of(name), C.family(name, "render_impl")
    impl = E.evaluate("render_impl", S, rays)
    parts = {}
    E.evaluate("render_impl", S, rays, parts)
    ih = np.flatnonzero(parts["hit"])
    assert ih.size >= 2 and np.array_equal(impl[:, 4] >= 0, parts["hit"])
    p = parts["p"][ih].astype(F)
    nrm = E.evaluate("sdf_normal", S, p)
    ao = E.evaluate("sdf_ao", S, np.concatenate([p, nrm], axis=1))
    sh = E.evaluate("sdf_shadow", S, C.shadow_rays(S, p)) if S["shadow"] else np.ones((len(p), 1), dtype=F)
    lit = E.evaluate("illuminate", S, np.concatenate([p, nrm, impl[ih, 4:5], ao, sh], axis=1))
    assert differing(lit, impl[ih, :3]) == 0, name
    miss = np.flatnonzero(~parts["hit"])
    assert (impl[miss, :3] == np.asarray(S["background"], dtype=F)).all() and (impl[miss, 4] == -1).all()
    if name.startswith("frame_"):                   # the families' own shading inputs are those values at the hit pixels
        x = C.family(name, "illuminate")
        assert differing(x[ih], np.concatenate([p, nrm, impl[ih, 4:5], ao, sh], axis=1)) == 0


@pytest.fixture(scope="module")
def outputs():
    out = {}
    for fn in E.FNS:
        for name in C.FAMILIES:
            parts = {}
            out[(fn, name)] = (E.evaluate(fn, C.scene_of(name), C.family(name, fn), parts), parts)
    return out


def test_families_say_something(outputs):
    """the conditions the GPU families rely on, from the model: conditions, not measurements"""
    tame = [n for n in C.FAMILIES if n != "specials"]
    hits = left = ran_out = 0
    exits = [0, 0, 0]
    parities, ids_in, ids_out = set(), 0, 0
    for name in tame:
        parts = outputs[("render_impl", name)][1]
        hits, left, ran_out = hits + int(parts["hit"].sum()), left + int(parts["left"].sum()), ran_out + int(parts["ran_out"].sum())
        ex = outputs[("sdf_shadow", name)][1]["exit"]
        for k in range(3):
            exits[k] += int((ex == k).sum())
        S, x = C.scene_of(name), C.family(name, "illuminate")
        ids = E.to_int(x[:, 6])
        ids_in, ids_out = ids_in + int(((ids >= 0) & (ids <= 7)).sum()), ids_out + int(((ids < 0) | (ids > 7)).sum())
        if not S["view"]:
            parities |= set(outputs[("illuminate", name)][1]["parity"].tolist())
        for fn in E.FNS:
            assert not np.isnan(C.family(name, fn)).any() and not np.isnan(outputs[(fn, name)][0]).any(), (fn, name, "NaN rows")
    assert hits >= 8 and left >= 8 and ran_out >= 8, (hits, left, ran_out)
    assert min(exits) >= 8, ("sdf_shadow exits: ran out, t > end, dark", exits)
    assert {0., 1.} <= parities, parities
    assert ids_in >= 8 and ids_out >= 8, (ids_in, ids_out)
    x = C.family("seeded", "illuminate")
    assert {float(F(v)) for v in C.IDS} <= set(x[:, 6].tolist()), "every id of IDS, the fractions included"
    length = np.sqrt((C.family("seeded", "render")[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
    assert (np.abs(length - 1) < 1e-6).sum() >= 256 and (np.abs(length - 1) > .05).sum() >= 256, "unit and non-unit directions"
    assert np.abs(C.family("seeded", "sdf")).max() <= 3 and len(C.scene_of("seeded")["program"]) == 32
    assert {len(C.family(n, "render")) for n in C.FRAMES} == {W * H}
    assert [C.scene_of(n)["shadow"] for n in C.FRAMES] == [1, 0, 0, 1, 0] and C.scene_of("frame_normals")["view"] == 1


def test_centres_and_specials_hold_their_rows(outputs):
    S = C.scene_of("centres")
    x = C.family("centres", "sdf")
    out = outputs[("sdf", "centres")][0]
    assert out[0].tolist() == [-.5, 2] and out[1, 1] == 3 and out[3, 1] == 4, "the sphere's centre; inside the cylinder; the torus's hole"
    assert out[3, 0] == F(.6) - F(.2), "on the torus's axis the inner root is of 0: |0 - R| - r"
    for I, rows, axis in ((S["program"][4], x[1:3], (0, 2)), (S["program"][6], x[3:5], (0, 1))):
        for k in axis:
            assert (rows[:, k] == I["offset"][k]).all(), "exactly on the axis"
    impl = outputs[("render_impl", "centres")][0]
    assert impl[0, 4] == 3 and impl[1, 4] == 5, "down the cylinder's axis onto its cap; through the torus's hole onto the box"
    for fn in E.FNS:
        win = E.WIDTHS[fn][0]
        x = C.family("specials", fn)
        assert len(x) == 1 + 6 * win
        for k in range(win):
            col = x[:, k]
            assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any() and (col == F(3e38)).any() and (col == F(1e-40)).any() \
                and ((col == 0) & np.signbit(col)).any(), (fn, k)
        out = outputs[(fn, "specials")][0]
        assert np.isfinite(out[0]).all(), fn
        if fn == "sdf_shadow":
            # sdf_shadow cannot return a NaN: against a NaN field value `t > end` and `d < .005` are false, t becomes NaN, and
            # min(umbra, NaN) = (NaN < umbra ? NaN : umbra) keeps umbra.  Its NaN rows march 20 steps and return 1, which the base row does not
            assert not np.isnan(out).any() and out[0, 0] == F(.05) and (out[np.isnan(x).any(axis=1), 0] == 1).all()
        else:
            assert np.isnan(out).any(axis=1).sum() >= 1, fn


def test_material_ids():
    S = C.scene_of("centres")
    assert E.to_int(np.array([np.nan, 1e10, -1e10, -.9, 2.9, -2.9, 7.9], dtype=F)).tolist() == [0, 2147483520, -2147483648, 0, 2, -2, 7]
    lit = E.evaluate("illuminate", S, np.array([[.25, .5, 1, 0, 1, 0, m, .5, .75] for m in (2, 2.9, 8, -1, np.nan, 0, -.5)], dtype=F))
    assert same_bits(lit[0], lit[1]).all() and (lit[0] > 0).all(), "toward zero"
    assert (lit[2] == 0).all() and (lit[3] == 0).all(), "outside 0..7: the zero colour (the port's choice)"
    assert same_bits(lit[4], lit[5]).all() and same_bits(lit[5], lit[6]).all(), "a NaN id and -.5 are id 0"
    nrm = E.evaluate("illuminate", dict(S, view=1), np.array([[.25, .5, 1, .1, .2, .3, 2, .5, .75]], dtype=F))
    assert nrm[0].tolist() == [float(F(.1)), float(F(.2)), float(F(.3))], "view 1: hit.normal"
