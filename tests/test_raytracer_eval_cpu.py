"""CPU tests of sbx_raytracer_eval's definition (tests/raytracer_eval_model.py; include/sbx.h): `render` over the
primary rays of every fixture scene is, after the app's sRGB step, the frame the reference's own headers rendered; with one bounce it
is the hand composition of the other three functions; the Python binding states the entry's widths; and the element families of
tests/raytracer_eval_cases.py meet the conditions under which the GPU tests say something."""
import numpy as np
import pytest

from tests import raytracer_eval_cases as C
from tests import raytracer_eval_model as E
from tests import raytracer_scene_model as M
from tests.model_common import F, ONE, same_bits
from tests.raytracer_builds_model import MAX_DIST, fresnel_factor, material


def differing(a, b):
    assert a.shape == b.shape, (a.shape, b.shape)
    return int((~same_bits(a, b)).reshape(len(a), -1).any(axis=-1).sum())


def test_widths_are_the_bindings():
    from shaderbox_amd import Renderer
    assert Renderer.EVAL_WIDTHS["raytracer"] == {"raytrace_iteration": (7, 8), "illuminate": (10, 3), "shadow": (3, 2), "render": (6, 4)}
    assert Renderer.EVAL_WIDTHS["raytracer"] == E.WIDTHS and tuple(Renderer.EVAL_WIDTHS["raytracer"]) == E.FNS, "in name-list order"
    assert callable(Renderer.raytracer_eval) and callable(Renderer.raytracer_eval_counted)


@pytest.mark.parametrize("name", list(M.scenes()))
def test_render_over_the_primary_rays_is_the_references_frame(name):
    w, h = M.scene_table()["size"]
    assert (w, h) == C.SIZE
    S = M.scenes()[name]
    out = E.evaluate("render", S, E.primary_rays(S, w, h))
    want = M.fixture(name)["frame"]
    assert differing(E.finish(out[:, :3]).reshape(h, w, 4), want) == 0, name
    masks = {}
    M.frame(S, w, h, masks)
    assert np.array_equal(out[:, 3].reshape(h, w), masks["depth"].astype(F)), "the depth is the scene model's"


@pytest.mark.parametrize("name", ["frame_mirrors", "frame_dirphong", "box_full", "box_spheres", "axes"])
def test_render_with_one_bounce_is_the_composition(name):
    """bounces = 1: colour = (1 - fresnel_factor(1, 1, dot(n, -rd))) * illuminate(eye = origin, hit), times .1 where the shadow test says
    so and the block's switch is on; depth = hit"""
    S = dict(C.scene_of(name), bounces=1)
    rays = C.family(name, 6)
    n = len(rays)
    with np.errstate(all="ignore"):
        hit = E.evaluate("raytrace_iteration", S, np.concatenate([rays, np.full((n, 1), -1, dtype=F)], axis=1))
        found = ~(hit[:, 0] >= MAX_DIST)
        ill = E.evaluate("illuminate", S, np.concatenate([rays[:, :3], hit[:, 2:5], hit[:, 5:8], hit[:, 1:2]], axis=1))
        sh = E.evaluate("shadow", S, np.ascontiguousarray(hit[:, 2:5]))
        ndotv = (hit[:, 5] * -rays[:, 3] + hit[:, 6] * -rays[:, 4]) + hit[:, 7] * -rays[:, 5]
        f = fresnel_factor(ONE, ONE, ndotv)
        want = np.zeros((n, 4), dtype=F)
        for k in range(3):
            c = F(0) + ((ONE - f) * ONE) * ill[:, k]
            if S["shadow"]:
                c = np.where(sh[:, 0] < sh[:, 1], c * F(0.1), c)
            want[:, k] = np.where(found, c, F(0))
        want[:, 3] = found
    got = E.evaluate("render", S, rays)
    assert differing(got, want) == 0, name
    assert found.any() and ((~found).any() or name in ("frame_mirrors", "box_full")), "hits, and misses where the scene is open"


def test_mat_to_ignore_and_material_ids():
    S = C.scene_of("axes")
    down = np.array([[1.5, 4, 0, 0, -1, 0, -1], [1.5, 4, 0, 0, -1, 0, 2], [1.5, 4, 0, 0, -1, 0, 2.9], [1.5, 4, 0, 0, -1, 0, 1],
                     [1.5, 4, 0, 0, 1, 0, -1]], dtype=F)
    out = E.evaluate("raytrace_iteration", S, down)
    assert out[0].tolist() == [2, 2, 1.5, 2, 0, 0, 1, 0], "the sphere's top"
    assert out[1].tolist() == out[2].tolist() == [4, 1, 1.5, 0, 0, 0, 1, 0], "the sphere ignored (2.9 converts toward zero): the floor"
    assert out[3].tolist() == out[0].tolist(), "planes are never skipped, whatever their material"
    assert out[4].tolist() == [float(F(1e8) + F(1e1)), -1, 0, 0, 0, 0, 0, 0], "no_hit"
    assert E.to_int(np.array([np.nan, 1e10, -1e10, -.9, 2.9, -2.9], dtype=F)).tolist() == [0, 2147483520, -2147483648, 0, 2, -2]
    lit = E.evaluate("illuminate", S, np.array([[0, 2, 5, 0, 0, 1, 0, 1, 0, m] for m in (0, 1, 8, -3)], dtype=F))
    assert lit[0].tolist() == [1, 1, 1], "mat_debug: flat"
    assert np.isfinite(lit[1]).all() and np.isnan(lit[2]).all() and same_bits(lit[2], lit[3]).all(), "outside 0..7: the zero material"
    assert material(S, np.array([8], dtype=np.int32))[3][0] == 0


@pytest.fixture(scope="module")
def outputs():
    return {(fn, name): E.evaluate(fn, C.scene_of(name), C.family(name, E.WIDTHS[fn][0])) for fn in E.FNS for name in C.FAMILIES}


def test_families_say_something(outputs):
    """the conditions the GPU families rely on, from the model: conditions, not measurements"""
    tame = [n for n in C.FAMILIES if n.startswith(("frame_", "box_"))]
    planes = spheres = misses = inside = 0
    for name in tame:
        S, x, out = C.scene_of(name), C.family(name, 7), outputs[("raytrace_iteration", name)]
        hit = ~(out[:, 0] >= MAX_DIST)
        with np.errstate(all="ignore"):
            only_planes = E.evaluate("raytrace_iteration", dict(S, spheres=[]), x)
        on_plane = hit & same_bits(out, only_planes).all(axis=1)
        planes, spheres, misses = planes + int(on_plane.sum()), spheres + int((hit & ~on_plane).sum()), misses + int((~hit).sum())
        for o, r, m in S["spheres"]:                   # the ray starts inside a sphere that it does not ignore and hits it: t0 < 0 -> t1
            d2 = sum((x[:, k].astype(np.float64) - float(o[k])) ** 2 for k in range(3))
            inside += int(((d2 < float(r) ** 2 * .98) & (E.to_int(x[:, 6]) != m) & hit & ~on_plane & (out[:, 1] == m)).sum())
    assert planes >= 100 and spheres >= 100 and misses >= 20, (planes, spheres, misses)
    assert inside >= 10, inside
    dark = sum(int((outputs[("shadow", n)][:, 0] < outputs[("shadow", n)][:, 1]).sum()) for n in tame)
    light = sum(int((~(outputs[("shadow", n)][:, 0] < outputs[("shadow", n)][:, 1])).sum()) for n in tame)
    assert dark >= 30 and light >= 30, (dark, light)
    depths = np.concatenate([outputs[("render", n)][:, 3] for n in tame])
    assert {0., 1., 2.} <= set(depths.tolist()) and (depths >= 3).any(), sorted(set(depths.tolist()))
    for fn in E.FNS:
        for name in tame:
            assert not np.isnan(C.family(name, E.WIDTHS[fn][0])).any() and not np.isnan(outputs[(fn, name)]).any(), (fn, name, "NaN rows")
    # the box families: the stated counts, unnormalised directions, every id of MATS
    assert [(len(C.scene_of(n)["planes"]), len(C.scene_of(n)["spheres"])) for n in ("box_full", "box_spheres")] == [(16, 16), (0, 7)]
    for name in ("box_full", "box_spheres"):
        x = C.family(name, 7)
        length = np.sqrt((x[:, 3:6].astype(np.float64) ** 2).sum(axis=1))
        assert len(x) == 1024 and length.min() >= .2 - 1e-6 and length.max() <= 2.5 + 1e-6 and (np.abs(length - 1) > .05).mean() > .8
        assert {float(F(m)) for m in C.MATS} <= set(C.family(name, 10)[:, 9].tolist())
        assert {float(F(m)) for m in C.MATS} <= set(x[:, 6].tolist())
    assert {len(C.family(n, 6)) for n in ("frame_mirrors", "frame_dirphong")} == {2304}
    assert (C.scene_of("frame_mirrors")["bounces"], C.scene_of("frame_dirphong")["light_type"], C.scene_of("frame_dirphong")["lighting"]) == (4, 2, 1)


def test_axes_and_specials_hold_their_rows(outputs):
    S = C.scene_of("axes")
    rays = np.array(C.AXES_RAYS, dtype=F)
    out = outputs[("raytrace_iteration", "axes")][:len(rays)]
    assert (out[:3, 2] == S["light"][0]).all() and (out[:3, 1] == 1).all(), "floor hits whose x is the light's: shadow_line.x == 0"
    for i in (3, 4, 5):                                # tangents: d2 == radius2 exactly, so t0 == t1 == tca
        o, r, _ = S["spheres"][0]
        rc = [F(o[k]) - rays[i, k] for k in range(3)]
        tca = (rc[0] * rays[i, 3] + rc[1] * rays[i, 4]) + rc[2] * rays[i, 5]
        d2 = ((rc[0] * rc[0] + rc[1] * rc[1]) + rc[2] * rc[2]) - tca * tca
        assert d2 == r * r, i
        assert (out[i, 0] == tca and out[i, 1] == 2) if i < 5 else out[i, 1] == 1, (i, "row 5's root is taken, then the floor is nearer")
    assert out[6, 1] == 2 and out[7, 1] == -1 and out[8, 1] == -1, "parallel to the plane; facing away from it"
    assert (out[9:12, 1] == 2).all() and (out[9:12, 0] > 0).all(), "from the centre: t0 < 0 -> t1"
    assert out[12, 1] == 2 and out[12, 0] == 1 and out[13, 1] == -1, "a zero direction: inside the sphere t1 = thc, outside a miss"
    sh = outputs[("shadow", "axes")]
    assert np.isfinite(sh).all() and (sh[:, 0] < sh[:, 1]).any() and (~(sh[:, 0] < sh[:, 1])).any()
    for fn in E.FNS:
        win = E.WIDTHS[fn][0]
        x = C.family("specials", win)
        coords = win - (1 if win in (7, 10) else 0)
        for k in range(coords):
            col = x[:, k]
            assert np.isnan(col).any() and (col == np.inf).any() and (col == -np.inf).any() and (col == F(3e38)).any() and (col == F(1e-40)).any() \
                and ((col == 0) & np.signbit(col)).any(), (fn, k)
        if win in (7, 10):
            assert np.isnan(x[:, -1]).any() and (x[:, -1] == F(1e10)).any() and (x[:, -1] == F(-1e10)).any()
        assert np.isnan(outputs[(fn, "specials")]).any() and np.isfinite(outputs[(fn, "specials")][0]).all(), fn
