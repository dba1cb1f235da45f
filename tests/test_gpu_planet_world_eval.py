"""GPU tests of sbx_planet_world_eval (include/sbx.h): sbx_planet_eval's eight functions under the caller's world, bit for bit
(NaN == NaN) against tests/planet_world_model.py's evaluate: every name over every fixture world under variants 0 and 1, through the
entry and its counted twin; the default block against sbx_planet_eval; elements built to leave the wave-wide `tame` set and blocks
outside the host's, with the counts showing both wave kinds ran; the shared checks of tests/eval_checks.py (ragged sizes, guard
words, alignment, a stream capture with the counted twin's refusal, the refusal loop); and the tie to the app: "render" over a fixture
frame's primary rays is that frame before linear_to_srgb."""
import ctypes
from functools import partial

import numpy as np
import pytest

from tests import planet_eval_model as E
from tests import planet_world_model as M
from tests.app_checks import assert_same, frame_cache
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F, get_primary_ray, point_cam

pytestmark = pytest.mark.gpu
FNS = E.FNS
RAY_FNS = ("render", "terrain_march")
W, H = M.SIZE


def primary_rays(Wd, w, h):
    """the primary rays of a world's camera at the pixel centres of a w x h frame, row by row -> [w * h, 6]"""
    fx, fy = np.broadcast_arrays((np.arange(w, dtype=F) + F(.5))[None, :], (np.arange(h, dtype=F) + F(.5))[:, None])
    pcx, pcy = point_cam(w, h, fx.ravel(), fy.ravel(), F(Wd["fov"]))
    rd = get_primary_ray(pcx, pcy, Wd["eye"], Wd["look_at"])
    out = np.empty((w * h, 6), dtype=F)
    out[:, :3] = np.array(Wd["eye"], dtype=F)
    out[:, 3:] = np.stack(rd, axis=1)
    return out


@frame_cache
def inputs(name, fn):
    """rays: every third primary ray of the world's own 48 x 27 frame (unit directions: the wave-wide test's set), then the families
    A-E of tests/planet_eval_model.py (other origins, lengths, specials, non-finite values: elements that leave it); points: A-E"""
    if fn in RAY_FNS:
        return np.concatenate([primary_rays(M.WORLDS[name], 48, 27)[::3], E.inputs(fn)], axis=0)
    return E.inputs(fn)


@frame_cache
def reference(name, fn):
    return M.evaluate(M.WORLDS[name], fn, inputs(name, fn))


def ev(r, fn, x, Wd):
    return r.planet_world_eval(fn, to_dev(x), M.as_aux(Wd))


def counted(r, fn, x, Wd):
    return r.planet_world_eval_counted(fn, to_dev(x), M.as_aux(Wd))


@pytest.mark.parametrize("name", sorted(M.WORLDS))
def test_every_name_over_a_fixture_world(renderer, variant_restored, name):
    for fn in FNS:
        x, want = inputs(name, fn), reference(name, fn)
        assert want.shape == (len(x), E.WIDTHS[fn][1])
        waves = (len(x) + 63) // 64
        for variant in (0, 1):
            renderer.set_variant(variant)
            assert differing(ev(renderer, fn, x, M.WORLDS[name]), want) == 0, (name, fn, variant)
            out, counts = counted(renderer, fn, x, M.WORLDS[name])
            assert differing(out, want) == 0, (name, fn, variant, "counted")
            assert sum(counts) == waves, (name, fn, counts)
            if variant == 1:
                assert counts == (0, waves), (name, fn, counts)
            elif fn in RAY_FNS:
                assert counts[0] > 0 and counts[1] > 0, (name, fn, counts, "both wave kinds ran")
            elif fn != "background":
                assert counts[0] > 0, (name, fn, counts)


def test_default_block_is_sbx_planet_eval(renderer):
    import shaderbox_amd
    for fn in FNS:
        x = E.inputs(fn)
        for t in (E.TIMES if fn in E.TIME_FNS else (0.0,)):
            want = renderer.planet_eval(fn, to_dev(x), t).cpu().numpy()
            got = renderer.planet_world_eval(fn, to_dev(x), shaderbox_amd.planet_world_default(t))
            assert differing(got, want) == 0, (fn, t)
            assert differing(ev(renderer, fn, x, M.default_world(t)), want) == 0, (fn, t, "the model's default block")
            assert differing(got, M.evaluate(M.default_world(t), fn, x)) == 0, (fn, t, "the model")


def test_camera_fields_are_not_read(renderer):
    Wd = dict(M.WORLDS["alpine"], eye=(F(np.nan),) * 3, look_at=(F(1e30), F(0), F(0)), fov=F(np.inf))
    for fn in ("render", "illuminate"):
        x = inputs("alpine", fn)[:256]
        out, counts = counted(renderer, fn, x, Wd)
        assert differing(out, reference("alpine", fn)[:256]) == 0, fn
        assert counts[0] > 0, (fn, counts)


def test_elements_and_blocks_that_leave_the_tame_set(renderer):
    """A wave of the world's own primary rays runs the guarded forms; the same wave with one direction of length 2, one far origin, one
    NaN, takes the plain form, and so does every wave of a block the host's test refuses (a reversed band, offsets of 1e6, cld_fuzzy
    0, an inf spin): the same bits as the model either way"""
    Wd = M.WORLDS["overcast"]
    rays = primary_rays(Wd, 48, 27)
    tr = {}
    M.render(Wd, [rays[:, k] for k in range(3)], [rays[:, 3 + k] for k in range(3)], tr)
    hit = np.flatnonzero(tr["atm"])[:64]
    assert len(hit) == 64
    tame = rays[hit]
    for fn in RAY_FNS:
        out, counts = counted(renderer, fn, tame, Wd)
        assert counts == (1, 0), (fn, counts)
        assert differing(out, M.evaluate(Wd, fn, tame)) == 0, fn
        for k, (col, v) in enumerate(((slice(3, 6), None), (0, 300.), (4, np.nan))):
            x = tame.copy()
            x[7 + k, col] = x[7 + k, col] * F(2) if v is None else F(v)
            out, counts = counted(renderer, fn, x, Wd)
            assert counts == (0, 1), (fn, k, counts)
            assert differing(out, M.evaluate(Wd, fn, x)) == 0, (fn, k)
    pts = E.inputs("clouds_density", "a")[:64].copy()
    assert counted(renderer, "clouds_density", pts, Wd)[1] == (1, 0)
    pts[5, 3] = F(1e-30)                                               # a height below 2^-60: band's dividend with an edge of 0
    out, counts = counted(renderer, "clouds_density", pts, Wd)
    assert counts == (0, 1) and differing(out, M.evaluate(Wd, "clouds_density", pts)) == 0, counts
    untame = dict(band=(.65, .35, .2), terrain_offset=(1e6, 0., 0.), cloud_offset=(0., -1e6, 0.), cld_fuzzy=0., spin_deg=np.inf, max_height=0.)
    for k, v in untame.items():
        Wu = M.world(.37, **{k: v})
        assert not M.tame(Wu), k
        for fn in ("render", "sdf_terrain_map_detail", "clouds_density"):
            x = tame if fn == "render" else E.inputs(fn, "a")[:64]
            out, counts = counted(renderer, fn, x, Wu)
            assert counts == (0, 1), (k, fn, counts)
            assert differing(out, M.evaluate(Wu, fn, x)) == 0, (k, fn)


@pytest.mark.parametrize("name", ["landing", "overcast"])
def test_render_over_a_frames_primary_rays_is_the_frame_before_srgb(renderer, name):
    Wd = M.WORLDS[name]
    lin = ev(renderer, "render", primary_rays(Wd, W, H), Wd).cpu().numpy()
    assert_same(E.linear_to_srgb(lin[:, :3]).reshape(H, W, 3), M.fixture(name)["frame"][..., :3], (name, "the reference's frame"))
    frame = renderer.render("planet_world", W, H, 0.0, aux=M.as_aux(Wd)).cpu().numpy()
    assert_same(E.linear_to_srgb(lin[:, :3]).reshape(H, W, 3), frame[..., :3], (name, "the app's frame"))
    assert 0 < int((lin[:, 3] > 0).sum()) < W * H


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    a = M.as_aux(M.WORLDS["alpine"])
    cases = []
    for fn in ("render", "sdf_terrain_normal", "sdf_terrain_map", "clouds_density"):
        x = inputs("alpine", fn)
        pick = np.resize(np.arange(len(x))[::-1], n)                   # from the specials backwards
        cases.append((fn, E.WIDTHS[fn], x[pick], reference("alpine", fn)[pick]))
    check_ragged(renderer, raw_call(renderer, "planet_world", lead=(ctypes.byref(a),)), cases, n)


def test_inside_a_stream_capture(renderer):
    a = M.as_aux(M.WORLDS["recoloured"])
    lead = (ctypes.byref(a),)
    twin = raw_call(renderer, "planet_world", lead=lead, counts=(ctypes.c_uint * 2)(7, 7))
    check_capture_replay(renderer, partial(raw_call(renderer, "planet_world", lead=lead), "render"), inputs("recoloured", "render"),
                         reference("recoloured", "render"), 4, refused_twin=partial(twin, "background"))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    rays = torch.from_numpy(E.family("a")[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 4), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr())
    good = M.as_aux(M.WORLDS["alpine"])
    g = ctypes.byref(good)
    assert lib.sbx_planet_world_eval(None, b"render", g, rp, op, 4, s) == -1
    bad_args = [(ctx, None, g, rp, op, 4, s), (ctx, b"render", None, rp, op, 4, s), (ctx, b"render", g, None, op, 4, s),
                (ctx, b"render", g, rp, None, 4, s), (ctx, b"density_func", g, rp, op, 4, s), (ctx, b"", g, rp, op, 4, s),
                (ctx, b"Render", g, rp, op, 4, s), (ctx, b"render", g, rp, op, (1 << 31) + 1, s)]
    keep = []
    for Wd in (M.world(terr_steps=0), M.world(terr_steps=513), M.world(cloud_steps=0), M.world(cloud_steps=257), M.world(shadow_steps=0),
               M.world(shadow_steps=33), M.world(reserved=(0, 1, 0, 0))):
        assert M.refused(Wd) is not None
        keep.append(M.as_aux(Wd))
        bad_args.append((ctx, b"render", ctypes.byref(keep[-1]), rp, op, 4, s))
    check_refusals(renderer, lib.sbx_planet_world_eval, lambda args: lib.sbx_debug_planet_world_eval(*args[:-1], (ctypes.c_uint * 2)(7, 7), s),
                   bad_args, out)
    for fn in FNS:
        assert lib.sbx_planet_world_eval(ctx, fn.encode(), g, None, None, 0, s) == 0       # n == 0 touches nothing
        assert renderer.planet_world_eval(fn, torch.zeros((0, E.WIDTHS[fn][0])), good).shape == (0, E.WIDTHS[fn][1])
    with pytest.raises(SbxError):
        renderer.planet_world_eval("density_func", rays, good)
    assert lib.sbx_debug_planet_world_eval(ctx, b"render", g, rp, op, 4, None, s) == -1    # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    before = renderer.stats()["render_launches"], renderer.planet_world_launches()
    assert differing(renderer.planet_world_eval("render", rays, good), M.evaluate(M.WORLDS["alpine"], "render", E.family("a")[:4])) == 0
    assert (renderer.stats()["render_launches"], renderer.planet_world_launches()) == before
