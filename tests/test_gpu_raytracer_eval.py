"""GPU tests of sbx_raytracer_eval (include/sbx.h): src/app_raytracer.h's raytrace_iteration, illuminate, shadow test
and render over the caller's elements under the caller's scene, bit for bit (NaN == NaN) against tests/raytracer_eval_model.py over the
families of tests/raytracer_eval_cases.py: the rays and hits of two fixture frames, seeded rays and points in two seeded scenes, exact
tangents and zero components where the witness records, NaN / inf / 3e38 / 1e-40 / -0 in every slot; a launch with one known re-run,
variants 1-3, a block whose camera is poisoned, ragged sizes with guard words, a stream capture, the refusals, and "render" tied to
SBX_APP_RAYTRACER_SCENE's frame.

No wave's form depends on its elements (csrc/kern_raytracer_eval.hip, at the top), so every wave of a default launch is counted:
witnessed + re-run == waves for every family, the specials included."""
import ctypes
from functools import partial

import numpy as np
import pytest

from shaderbox_amd import Renderer
from tests import raytracer_eval_cases as C
from tests import raytracer_eval_model as E
from tests import raytracer_scene_model as M
from tests.app_checks import assert_same, frame_cache
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu
W, H = C.SIZE
WIDTHS = Renderer.EVAL_WIDTHS["raytracer"]
FNS = tuple(WIDTHS)

family = frame_cache(lambda name, win: C.family(name, win))
block = frame_cache(lambda name: M.to_block(C.scene_of(name)))
reference = frame_cache(lambda fn, name: E.evaluate(fn, C.scene_of(name), family(name, WIDTHS[fn][0])))


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("name", C.FAMILIES)
def test_against_the_model(renderer, fn, name):
    x, a = family(name, WIDTHS[fn][0]), block(name)
    want = reference(fn, name)
    assert want.shape == (len(x), WIDTHS[fn][1])
    assert differing(renderer.raytracer_eval(fn, to_dev(x), a), want) == 0, (fn, name)
    out, (witnessed, rerun) = renderer.raytracer_eval_counted(fn, to_dev(x), a)
    assert differing(out, want) == 0, (fn, name, "counted")
    waves = (len(x) + 63) // 64
    print(fn, name, "waves", waves, "witnessed", witnessed, "re-run", rerun, "NaN rows", int(np.isnan(want).any(axis=1).sum()))
    assert witnessed + rerun == waves, (fn, name, witnessed, rerun)
    if name in ("axes", "specials") and fn != "raytrace_iteration":
        assert rerun >= 1, (fn, name, "a zero component, a root of 0, a NaN: the wave records")


def test_one_known_rerun_among_three_waves(renderer):
    """waves 0 and 2: 64 seeded rays each; wave 1: 63 seeded rays and, at lane 17, the ray tangent to the sphere of "axes" (d2 == radius2:
    the root of 0 is outside the witness's interval).  The seeded rays are deterministic and record nothing — the counted run of the
    three waves before the tangent ray is put in says so, and so would any seed: a record needs an exact zero, a denormal, an inf or a NaN."""
    S, a = C.scene_of("axes"), block("axes")
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(-1, 1, size=(192, 3)) * [3, 1.5, 3] + [0, 2, 1], rng.normal(size=(192, 3))], axis=1).astype(F)
    out, counts = renderer.raytracer_eval_counted("render", to_dev(x), a)
    assert counts == (3, 0), ("the seeded rays record nothing", counts)
    assert differing(out, E.evaluate("render", S, x)) == 0
    x[64 + 17] = C.recording_ray()
    out, counts = renderer.raytracer_eval_counted("render", to_dev(x), a)
    assert counts == (2, 1), counts
    assert differing(out, E.evaluate("render", S, x)) == 0


def test_variants_same_bits(renderer, variant_restored):
    reran = 0
    for fn in FNS:
        for name in ("frame_mirrors", "frame_dirphong", "axes", "specials"):
            x, a = family(name, WIDTHS[fn][0]), block(name)
            for variant in (1, 2, 3):
                renderer.set_variant(variant)
                out, counts = renderer.raytracer_eval_counted(fn, to_dev(x), a)
                assert differing(out, reference(fn, name)) == 0, (fn, name, variant)
                if variant != 2:
                    assert counts == (0, 0), (fn, name, variant, counts)
                else:
                    assert counts[0] + counts[1] == (len(x) + 63) // 64, (fn, name, counts)
                    reran += counts[1] if name.startswith("frame_") else 0
            renderer.set_variant(0)
    assert reran > 0, "under the witness's test edge some wave of a frame re-runs"


def test_the_camera_of_the_block_is_not_read(renderer):
    for name in ("frame_mirrors", "box_spheres"):
        S = dict(C.scene_of(name), eye=(F(np.nan),) * 3, look_at=(F(np.inf),) * 3, fov=F(-3e38))
        a = M.to_block(S)
        assert np.isnan(a.eye[0]) and np.isinf(a.look_at[2]) and a.fov < -1e38
        for fn in FNS:
            out, counts = renderer.raytracer_eval_counted(fn, to_dev(family(name, WIDTHS[fn][0])), a)
            assert differing(out, reference(fn, name)) == 0, (fn, name)
            assert counts[0] + counts[1] == (len(out) + 63) // 64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; in and out at an odd dword offset (4 bytes off a 16-byte boundary);
    every output width"""
    name = "frame_mirrors"
    pick = np.resize(np.arange(W * H), n)
    cases = [(fn, WIDTHS[fn], family(name, WIDTHS[fn][0])[pick], reference(fn, name)[pick]) for fn in FNS]
    check_ragged(renderer, raw_call(renderer, "raytracer", lead=(ctypes.byref(block(name)),)), cases, n)


def test_inside_a_stream_capture(renderer):
    """one capture, replayed twice, the second time over the reversed rays in the same buffers; the counted twin refuses the capturing stream"""
    name = "frame_mirrors"
    a = ctypes.byref(block(name))
    twin = raw_call(renderer, "raytracer", lead=(a,), counts=(ctypes.c_uint * 2)(7, 7))
    check_capture_replay(renderer, partial(raw_call(renderer, "raytracer", lead=(a,)), "render"), family(name, 6)[:1024],
                         reference("render", name)[:1024], 4, refused_twin=partial(twin, "render"))


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    name = "frame_mirrors"
    a = block(name)
    rays = torch.from_numpy(family(name, 6)[:4].copy()).to(renderer.tdev)
    wide = torch.zeros((4, 10), dtype=torch.float32, device=renderer.tdev)
    out = torch.full((4, 8), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op, ap = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.byref(a)
    assert lib.sbx_raytracer_eval(None, b"render", ap, rp, op, 4, s) == -1
    bad_args = [(ctx, None, ap, rp, op, 4, s), (ctx, b"render", ap, None, op, 4, s), (ctx, b"render", ap, rp, None, 4, s),
                (ctx, b"render", None, rp, op, 4, s), (ctx, b"shadow", None, rp, op, 0, s),
                (ctx, b"intersect_sphere", ap, rp, op, 4, s), (ctx, b"", ap, rp, op, 4, s), (ctx, b"Render", ap, rp, op, 4, s),
                (ctx, b"render", ap, rp, op, (1 << 31) + 1, s)]
    texts = {}
    for field, values, text in (("n_planes", (-1, 17), b"n_planes and n_spheres must lie in 0..16"), ("n_spheres", (-1, 17), b"n_planes and n_spheres must lie in 0..16"),
                                ("bounces", (0, 9), b"bounces must lie in 1..8"), ("light_type", (0, 3), b"light_type must be 1 (LIGHT_POINT) or 2 (LIGHT_DIR)"),
                                ("lighting", (-1, 2), b"lighting must be 0 (Cook-Torrance) or 1 (Phong)"), ("shadow", (-1, 2), b"shadow must be 0 or 1")):
        for v in values:
            b = M.to_block(C.scene_of(name))
            setattr(b, field, v)
            for n in (4, 0):                                                               # the block is checked whatever n is
                bad_args.append((ctx, b"render", ctypes.byref(b), rp, op, n, s))
                texts[len(bad_args) - 1] = b"raytracer scene: " + text
    check_refusals(renderer, lib.sbx_raytracer_eval, lambda args: lib.sbx_debug_raytracer_eval(*args[:-1], (ctypes.c_uint * 2)(7, 7), s), bad_args, out)
    for i, text in texts.items():                                                          # the app's texts
        assert lib.sbx_raytracer_eval(*bad_args[i]) == -1 and text in lib.sbx_last_error(ctx), (i, text)
        with pytest.raises(SbxError) as app:
            renderer.render("raytracer_scene", W, H, 0.0, aux=bad_args[i][2]._obj)
        assert text.decode() in str(app.value)
    scene_launches, launches = renderer.raytracer_scene_launches(), renderer.stats()["render_launches"]
    for fn, (win, wout) in WIDTHS.items():
        assert lib.sbx_raytracer_eval(ctx, fn.encode(), ap, None, None, 0, s) == 0        # n == 0 touches nothing
        assert renderer.raytracer_eval(fn, torch.zeros((0, win)), a).shape == (0, wout)
        assert renderer.raytracer_eval_counted(fn, torch.zeros((0, win)), a)[1] == (0, 0)
        assert renderer.raytracer_eval(fn, wide[:, :win], a).shape == (4, wout)
    with pytest.raises(SbxError):
        renderer.raytracer_eval("intersect_plane", rays, a)
    assert lib.sbx_debug_raytracer_eval(ctx, b"render", ap, rp, op, 4, None, s) == -1     # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert differing(renderer.raytracer_eval("render", rays, a), reference("render", name)[:4]) == 0
    assert renderer.stats()["render_launches"] == launches and renderer.raytracer_scene_launches() == scene_launches, "not a render"


@pytest.mark.parametrize("name", list(M.scenes()))
def test_render_over_the_primary_rays_is_the_apps_frame(renderer, name):
    """"render" over a frame's primary rays, then the model's sRGB step: SBX_APP_RAYTRACER_SCENE's frame, which is the fixture's"""
    S = M.scenes()[name]
    a = M.to_block(S)
    out = renderer.raytracer_eval("render", to_dev(E.primary_rays(S, W, H)), a).cpu().numpy()
    frame = renderer.render("raytracer_scene", W, H, 0.0, aux=a).cpu().numpy()
    assert_same(E.finish(out[:, :3]).reshape(H, W, 4), frame, name)
    assert_same(frame, M.fixture(name)["frame"], (name, "fixture"))
