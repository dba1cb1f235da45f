"""GPU tests of sbx_vinyl_eval (include/sbx.h): APP_VINYL's field, normal, soft shadow, shading and trace over the
caller's elements under the caller's deck, bit for bit (NaN == NaN) against tests/vinyl_deck_model.py: the rays and hit points of a
frame, seeded points and rays in a box around the deck, axis-aligned rays and points on the surfaces (exact-zero normal components,
points on the spindle's axis where the witness records), a family of NaN / inf / 1e5 values and the origin where hit.origin / r is
0 / 0, launches that mix tame and untame waves, an untame deck, ragged sizes with guard words, variants 1-3, a stream capture, the
refusals, "render" tied to SBX_APP_VINYL_DECK's frame, and host/sbx_render's --vinyl-view."""
import ctypes
from functools import partial

import numpy as np
import pytest

from shaderbox_amd import Renderer
from tests import vinyl_deck_model as M
from tests.app_checks import assert_same, frame_cache, run_sbx_render
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu
W, H = M.SIZE
WIDTHS = Renderer.EVAL_WIDTHS["vinyl"]
FNS = tuple(WIDTHS)
# the deck of the axis-aligned family: no rotation at all, so that the platter's faces are the planes y = +-.05 of the world
FLAT = M.deck(0., platter_deg=0., platter_tilt_deg=0., arm_tilt_deg=0., sun_dir=(0., 1., 0.))
DECK_OF = {"frame": M.DECKS["scratch"], "box": M.DECKS["coloured"], "axes": FLAT, "specials": M.DECKS["dusk"]}


def frame_rays(D, w, h):
    fx, fy = M.frame_coords(w, h)
    ro, rd = M.primary_rays(D, w, h, fx, fy)
    n = rd[0].size
    return np.stack([np.full(n, ro[0]), np.full(n, ro[1]), np.full(n, ro[2]), rd[0], rd[1], rd[2]], axis=1).astype(F)


def shape(x, win, rng, mats):
    """a family's [n, 6] (point, second vector) as inputs of width win: the point; both; or eye = the second vector, hit = the point, a material id"""
    if win == 3:
        return np.ascontiguousarray(x[:, :3])
    if win == 6:
        return x
    return np.concatenate([x[:, 3:], x[:, :3], rng.choice(np.asarray(mats, dtype=F), size=(len(x), 1))], axis=1).astype(F)


def family(name, win):
    """inputs [n, win] of a family; the deck they are meant for is DECK_OF[name]"""
    rng = np.random.default_rng({"frame": 1, "box": 2, "axes": 3, "specials": 4}[name])
    if name == "frame":
        # the frame's primary rays; as points, its hit points (the march's end for a miss); as shading inputs, eye, hit point and material
        D = DECK_OF[name]
        rays = frame_rays(D, W, H)
        if win == 6:
            return rays
        parts = {}
        t = M.render(M.scene_of(D), tuple(rays[0, :3]), tuple(rays[:, 3 + k] for k in range(3)), parts)[1]
        p = np.where(parts["hit"][:, None], parts["p"], rays[:, :3] + rays[:, 3:] * t[:, None]).astype(F)
        if win == 3:
            return p
        return np.concatenate([rays[:, :3], p, np.where(parts["hit"], parts["mat"], 0).astype(F)[:, None]], axis=1).astype(F)
    if name == "box":
        n = 1024
        o = rng.uniform(-9, 9, size=(n, 3)) * [1, .35, 1] + [0, .5, 0]
        d = rng.normal(size=(n, 3)) * rng.uniform(.2, 2.5, size=(n, 1))
        if win == 7:
            d = rng.uniform(-9, 9, size=(n, 3)) + [0, 8, 0]                  # eyes above the deck
        return shape(np.concatenate([o, d], axis=1).astype(F), win, rng, [-3, 0, 1, 1, 2, 2, 2.9, 3, 4, 5, 6, 100])
    if name == "axes":
        # FLAT: on the platter's top face per material ring, on its rim, on the spindle's axis and sphere centre, on the base's axis,
        # the origin (hit.origin / r is 0 / 0), a defect's centre; second vector: straight down, straight up, along x, zero
        pts = [[4.5, .05, 0], [0, .05, 4.5], [2.5, .05, 0], [0, .05, -2.5], [1.7, .05, 0], [0, .0825, .3], [0, .3, 0], [0, .6, 0], [0, 0, 0],
               [5.9, 0, 0], [-6.05, 0, 0], [-7, 1.25, -5], [-7, 0, -5], [3., 2., 0], [0, 3., 0], [-2, .8, 4]]
        second = [[0, -1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 0]]
        x = np.array([p + second[(i // len(pts)) % 4] for i, p in enumerate(pts * 4)], dtype=F)
        if win == 7:
            x[:, 3:] = x[:, :3] + np.array([second[1], second[1], [0, 2, 0], [0, 5, 0]], dtype=F)[(np.arange(len(x)) // len(pts)) % 4]
        return shape(x, win, rng, [1, 2, 3, 4, 5])
    big, nan, inf = 3e38, np.nan, np.inf
    rows = [[0, 0, 0, 0, 0, 0], [0, 3, 0, 0, -1, 0], [0, 3, 0, nan, -1, 0], [0, 3, 0, 0, nan, 0], [nan, 3, 0, 0, -1, 0], [0, 3, 0, inf, -1, 0],
            [0, 3, 0, 0, -inf, 0], [inf, 3, 0, 0, -1, 0], [0, -inf, 1, 0, -1, 0], [0, inf, 1, 0, -1, 0], [big, 3, 0, 0, -1, 0], [0, 3, 0, big, -big, 0],
            [0, 3, 0, 0, -1e-40, 0], [0, 3, 0, 0, -1e5, 0], [1e5, 1, 0, -1, 0, 0], [0, 1e5, 0, 0, -1, 0], [0, 1e19, 0, 0, -1, 0],
            [4, 3, 0, 0, -1, 0], [4, 9999, 0, 0, -9999, 0], [-0., 3, -0., -0., -1, -0.]]
    x = np.array(rows, dtype=F)
    if win == 7:                                   # the hit stays near the deck for half of them, so that the odd value is the eye's
        with np.errstate(all="ignore"):            # (3e38 * -3 is an inf on purpose)
            x = np.concatenate([x, np.concatenate([x[:, 3:] * F(-3), x[:, :3] * F(.001)], axis=1)], axis=0).astype(F)
        x[:3, :3] = 0                              # hit.origin = 0 under every material: r = 0, B = 0 / 0
        return np.concatenate([x[:, 3:], x[:, :3], (np.arange(len(x)) % 7).astype(F)[:, None]], axis=1).astype(F)
    return shape(x, win, rng, [1])


def model(fn, D, x):
    """the model over elements x[n, win] -> [n, wout]"""
    S = M.scene_of(D)
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        a, b = tuple(x[:, k] for k in range(3)), tuple(x[:, k] for k in range(3, 6)) if x.shape[1] >= 6 else None
        if fn == "sdf":
            return np.stack(M.sdf(S, *a), axis=1).astype(F)
        if fn == "sdf_normal":
            return np.stack(M.sdf_normal(S, a), axis=1).astype(F)
        if fn == "sdf_shadow":
            return M.sdf_shadow(S, a, b)[:, None]
        if fn == "illuminate":
            return M.illuminate(S, a, b, M.to_int(x[:, 6]))
        rgb, t, mat = M.render(S, a, b)
        return np.concatenate([rgb, t[:, None], mat[:, None]], axis=1).astype(F)


reference = frame_cache(lambda fn, name: model(fn, DECK_OF[name], family(name, WIDTHS[fn][0])))


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("name", ["frame", "box", "axes", "specials"])
def test_against_the_model(renderer, fn, name):
    x, a = family(name, WIDTHS[fn][0]), M.as_aux(DECK_OF[name])
    want = reference(fn, name)
    assert want.shape == (len(x), WIDTHS[fn][1])
    assert differing(renderer.vinyl_eval(fn, to_dev(x), a), want) == 0, (fn, name)
    out, (witnessed, rerun) = renderer.vinyl_eval_counted(fn, to_dev(x), a)
    assert differing(out, want) == 0, (fn, name, "counted")
    waves = (len(x) + 63) // 64
    print(fn, name, "waves", waves, "witnessed", witnessed, "re-run", rerun, "NaN rows", int(np.isnan(want).any(axis=1).sum()))
    if name == "specials":
        assert witnessed == rerun == 0, (fn, "a wave with an untame element takes the plain form", witnessed, rerun)
    else:
        assert witnessed + rerun == waves, (fn, name, witnessed, rerun)
    if name == "axes" and fn == "sdf_normal":      # flat faces: exact zeros
        flat = want[:5]
        assert (flat[:, 0] == 0).all() and (flat[:, 2] == 0).all() and (flat[:, 1] > .999).all(), flat
    if name == "frame" and fn == "render":
        assert (want[:, 4] > 0).mean() > .4 and len(set(want[:, 4])) == 6, "every material and the background are among the frame's rays"


def test_tame_and_untame_waves_in_one_launch(renderer):
    """wave 0: 64 seeded points; wave 1: 64 with one NaN among them; wave 2: 64 seeded points; wave 3: 5 points beyond 1e4.  Waves 0 and 2
    are counted (culled, witnessed), 1 and 3 take the plain form; the bits are the model's as if apart"""
    D = DECK_OF["box"]
    for fn in ("sdf", "sdf_shadow", "render"):
        win = WIDTHS[fn][0]
        box = family("box", win)
        x = np.concatenate([box[:64], box[64:128], box[128:192], box[192:197] * F(3e4)], axis=0)
        x[64 + 17, 1] = np.nan
        out, counts = renderer.vinyl_eval_counted(fn, to_dev(x), M.as_aux(D))
        assert counts[0] + counts[1] == 2, (fn, counts)
        assert differing(out, model(fn, D, x)) == 0, fn


def test_an_untame_deck_takes_the_plain_form(renderer):
    """a NaN sun, an inf angle, a sun beyond 1e4: no wave is witnessed or culled, the bits are the model's"""
    x = family("box", 6)[:256]
    for D in (M.deck(.37, sun_dir=(np.nan, 1., 0.)), M.deck(.37, platter_deg=np.inf), M.deck(.37, sun_dir=(0., 2e4, 0.))):
        for fn in ("sdf", "sdf_shadow", "render"):
            xi = np.ascontiguousarray(x[:, :WIDTHS[fn][0]])
            out, counts = renderer.vinyl_eval_counted(fn, to_dev(xi), M.as_aux(D))
            assert counts == (0, 0), (fn, counts)
            assert differing(out, model(fn, D, xi)) == 0, fn


def test_the_camera_of_the_deck_is_not_read(renderer):
    x = family("box", 6)[:128]
    D = dict(M.DECKS["coloured"])
    want = renderer.vinyl_eval("render", to_dev(x), M.as_aux(D)).cpu().numpy()
    D.update(eye=(F(np.nan),) * 3, look_at=(F(np.inf),) * 3, fov=F(-3e38))
    out, counts = renderer.vinyl_eval_counted("render", to_dev(x), M.as_aux(D))
    assert differing(out, want) == 0 and counts[0] + counts[1] == 2


def test_variants_same_bits(renderer, variant_restored):
    for fn in FNS:
        for name in ("frame", "axes", "specials"):
            x, a = family(name, WIDTHS[fn][0]), M.as_aux(DECK_OF[name])
            for variant in (1, 2, 3):
                renderer.set_variant(variant)
                out, counts = renderer.vinyl_eval_counted(fn, to_dev(x), a)
                assert differing(out, reference(fn, name)) == 0, (fn, name, variant)
                if variant != 2:
                    assert counts == (0, 0), (fn, name, variant, counts)
            renderer.set_variant(0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; in and out at an odd dword offset (4 bytes off a 16-byte boundary);
    every output width"""
    a = M.as_aux(DECK_OF["frame"])
    pick = np.resize(np.arange(len(family("frame", 6))), n)
    cases = [(fn, WIDTHS[fn], family("frame", WIDTHS[fn][0])[pick], reference(fn, "frame")[pick]) for fn in FNS]
    check_ragged(renderer, raw_call(renderer, "vinyl", lead=(ctypes.byref(a),)), cases, n)


def test_inside_a_stream_capture(renderer):
    """one capture, replayed twice, the second time over other rays in the same buffers; the counted twin refuses the capturing stream"""
    a = ctypes.byref(M.as_aux(DECK_OF["frame"]))
    twin = raw_call(renderer, "vinyl", lead=(a,), counts=(ctypes.c_uint * 2)(7, 7))
    check_capture_replay(renderer, partial(raw_call(renderer, "vinyl", lead=(a,)), "render"), family("frame", 6)[:1024],
                         reference("render", "frame")[:1024], 5, refused_twin=partial(twin, "sdf"))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    a = M.as_aux(DECK_OF["frame"])
    rays = torch.from_numpy(family("frame", 6)[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 5), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op, ap = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.byref(a)
    assert lib.sbx_vinyl_eval(None, b"render", ap, rp, op, 4, s) == -1
    bad_args = [(ctx, None, ap, rp, op, 4, s), (ctx, b"render", ap, None, op, 4, s), (ctx, b"render", ap, rp, None, 4, s),
                (ctx, b"render", None, rp, op, 4, s), (ctx, b"sdf", None, rp, op, 4, s), (ctx, b"illuminate", None, rp, op, 0, s),
                (ctx, b"render_scene", ap, rp, op, 4, s), (ctx, b"", ap, rp, op, 4, s), (ctx, b"Sdf", ap, rp, op, 4, s),
                (ctx, b"shadowmarch", ap, rp, op, 4, s), (ctx, b"render", ap, rp, op, (1 << 31) + 1, s)]
    check_refusals(renderer, lib.sbx_vinyl_eval, lambda args: lib.sbx_debug_vinyl_eval(*args[:-1], (ctypes.c_uint * 2)(7, 7), s), bad_args, out)
    for fn, (win, wout) in WIDTHS.items():
        assert lib.sbx_vinyl_eval(ctx, fn.encode(), ap, None, None, 0, s) == 0            # n == 0 touches nothing
        assert renderer.vinyl_eval(fn, torch.zeros((0, win)), a).shape == (0, wout)
    with pytest.raises(SbxError):
        renderer.vinyl_eval("render_scene", rays, a)
    assert lib.sbx_debug_vinyl_eval(ctx, b"render", ap, rp, op, 4, None, s) == -1         # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    before = renderer.stats()["render_launches"]                                          # not a render
    assert differing(renderer.vinyl_eval("render", rays, a), reference("render", "frame")[:4]) == 0
    assert renderer.stats()["render_launches"] == before


@pytest.mark.parametrize("name", ["scratch", "coloured", "dusk"])
def test_render_over_the_primary_rays_is_the_apps_frame(renderer, name):
    """"render" over a frame's primary rays, then linear_to_srgb from the model: SBX_APP_VINYL_DECK's frame"""
    D = M.DECKS[name]
    out = renderer.vinyl_eval("render", to_dev(frame_rays(D, W, H)), M.as_aux(D)).cpu().numpy()
    frame = renderer.render("vinyl_deck", W, H, 0.0, aux=M.as_aux(D)).cpu().numpy()
    assert_same(M.finish(out[:, :3]).reshape(H, W, 4), frame, name)
    assert_same(frame, M.fixture(name)["frame"], (name, "fixture"))


def test_vinyl_view_of_sbx_render(renderer, tmp_path):
    """host/sbx_render --vinyl-view with the close-up camera and the coloured deck's flags writes what SBX_APP_VINYL_DECK renders with
    that camera in its block; with the shipped camera and no flags, SBX_APP_VINYL's frame of --time"""
    c = lambda v: ",".join(repr(float(x)) for x in v)  # noqa: E731
    D = dict(M.DECKS["coloured"])
    D.update(eye=(F(-2), F(1.5), F(5.5)), look_at=(F(-1.5), F(0), F(0)), fov=F(.8))
    view = ["--vinyl-view", str(W), str(H)] + [repr(float(v)) for v in D["eye"]] + [repr(float(v)) for v in D["look_at"]]
    flags = view + ["--fov", repr(float(D["fov"])), "--groove-color", c(D["groove_color"]), "--dead-wax-color", c(D["dead_wax_color"]),
                    "--label-color", c(D["label_color"]), "--logo-color", c(D["logo_color"]), "--shiny-color", c(D["shiny_color"]),
                    "--ro-spec", repr(float(D["ro_spec"])), "--a-x", repr(float(D["a_x"])), "--a-y", repr(float(D["a_y"])),
                    "--shininess", repr(float(D["shininess"]))]
    want = renderer.render("vinyl_deck", W, H, 0.0, aux=M.as_aux(D)).cpu().numpy()
    assert_same(want, M.frame(M.scene_of(D), W, H), "the deck app with the close-up camera")
    assert_same(run_sbx_render(tmp_path, "vinyl", W, H, .37, flags=flags), want, "--vinyl-view, coloured close-up")
    shipped = ["--vinyl-view", str(W), str(H), "0", "5.75", "6.75", "0", "-2.5", "0"]
    assert_same(run_sbx_render(tmp_path, "vinyl", W, H, 2.5, flags=shipped), renderer.render("vinyl", W, H, 2.5).cpu().numpy(), "--vinyl-view, shipped")
