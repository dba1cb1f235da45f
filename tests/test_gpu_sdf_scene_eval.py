"""GPU tests of sbx_sdf_scene_eval (include/sbx.h): src/app_sdf_ao.h's sdf_normal, sdf_ao, sdf_shadow, illuminate,
render_impl and render, with sdf(pos) the caller's program, over the caller's elements under the caller's block, bit for bit (NaN == NaN)
against tests/sdf_scene_eval_model.py over the families of tests/sdf_scene_eval_cases.py: the rays and hits of five frames, seeded
elements in a seeded 32-instruction scene, centres and axes where the witness records, NaN / inf / 3e38 / 1e-40 / -0 in every slot; a
launch with one known re-run, variants 1-3, a block whose camera is poisoned, ragged sizes with guard words, a stream capture, the
refusals, and the ties to sbx_sdf_eval, to SBX_APP_SDF_SCENE's frame and of "render_impl" to the chain of the other functions.

No wave's form depends on its elements or on the block (csrc/kern_sdf_scene_eval.hip, at the top), so every wave of a default launch is
counted: witnessed + re-run == waves for every family, the specials included.  "illuminate" evaluates no field and takes no root: no
wave of it can record, and the test says so (re-run == 0) where the other names must re-run over "centres" and "specials"."""
import ctypes
from functools import partial

import numpy as np
import pytest

from shaderbox_amd import Renderer
from tests import sdf_scene_eval_cases as C
from tests import sdf_scene_eval_model as E
from tests import sdf_scene_model as M
from tests.app_checks import assert_same, frame_cache
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu
W, H = C.SIZE
WIDTHS = Renderer.EVAL_WIDTHS["sdf_scene"]
FNS = tuple(WIDTHS)

family = frame_cache(lambda name, fn: C.family(name, fn))
block = frame_cache(lambda name: M.as_aux(C.scene_of(name)))
reference = frame_cache(lambda fn, name: E.evaluate(fn, C.scene_of(name), family(name, fn)))


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("name", C.FAMILIES)
def test_against_the_model(renderer, fn, name):
    x, a = family(name, fn), block(name)
    want = reference(fn, name)
    assert want.shape == (len(x), WIDTHS[fn][1])
    assert differing(renderer.sdf_scene_eval(fn, to_dev(x), a), want) == 0, (fn, name)
    out, (witnessed, rerun) = renderer.sdf_scene_eval_counted(fn, to_dev(x), a)
    assert differing(out, want) == 0, (fn, name, "counted")
    waves = (len(x) + 63) // 64
    print(fn, name, "waves", waves, "witnessed", witnessed, "re-run", rerun, "NaN rows", int(np.isnan(want).any(axis=1).sum()))
    assert witnessed + rerun == waves, (fn, name, witnessed, rerun)
    if not C.roots(fn):
        assert rerun == 0, (fn, name, "no root, nothing to record")
    elif name in ("centres", "specials"):
        assert rerun >= 1, (fn, name, "a root of 0, a NaN: the wave records")


def test_one_known_rerun_among_three_waves(renderer):
    """waves 0 and 2: 64 seeded rays each; wave 1: 63 seeded rays and, at lane 17, the ray down the cylinder's axis of "centres" (every
    sample's radial root is of 0, outside the witness's interval).  The seeded rays are deterministic and record nothing — the counted
    run of the three waves before that ray is put in says so: a record needs an exact zero, a denormal, an inf or a NaN."""
    S, a = C.scene_of("centres"), block("centres")
    rng = np.random.default_rng(11)
    o = rng.uniform(-1, 1, size=(3, 3)) * [3, 1, 3] + [0, 3, 0]
    aim = rng.uniform(-1, 1, size=(192, 3)) * [3, .5, 3] + [0, .5, 0] - np.repeat(o, 64, axis=0)
    x = np.concatenate([np.repeat(o, 64, axis=0), aim / np.linalg.norm(aim, axis=1, keepdims=True)], axis=1).astype(F)
    out, counts = renderer.sdf_scene_eval_counted("render", to_dev(x), a)
    assert counts == (3, 0), ("the seeded rays record nothing", counts)
    assert differing(out, E.evaluate("render", S, x)) == 0
    x[64 + 17] = C.recording_ray()
    out, counts = renderer.sdf_scene_eval_counted("render", to_dev(x), a)
    assert counts == (2, 1), counts
    assert differing(out, E.evaluate("render", S, x)) == 0


def test_variants_same_bits(renderer, variant_restored):
    reran = 0
    for fn in FNS:
        for name in ("frame_shadow", "frame_normals", "centres", "specials"):
            x, a = family(name, fn), block(name)
            for variant in (1, 2, 3):
                renderer.set_variant(variant)
                out, counts = renderer.sdf_scene_eval_counted(fn, to_dev(x), a)
                assert differing(out, reference(fn, name)) == 0, (fn, name, variant)
                if variant != 2:
                    assert counts == (0, 0), (fn, name, variant, counts)
                else:
                    assert counts[0] + counts[1] == (len(x) + 63) // 64, (fn, name, counts)
                    reran += counts[1] if name.startswith("frame_") else 0
            renderer.set_variant(0)
    assert reran > 0, "under the witness's test edge some wave of a frame re-runs"


def test_the_camera_of_the_block_is_not_read(renderer):
    for name in ("frame_short", "centres"):
        S = dict(C.scene_of(name), eye=(F(np.nan),) * 3, look_at=(F(np.inf),) * 3, fov=F(-3e38))
        a = M.as_aux(S)
        assert np.isnan(a.eye[0]) and np.isinf(a.look_at[2]) and a.fov < -1e38
        for fn in FNS:
            out, counts = renderer.sdf_scene_eval_counted(fn, to_dev(family(name, fn)), a)
            assert differing(out, reference(fn, name)) == 0, (fn, name)
            assert counts[0] + counts[1] == (len(out) + 63) // 64


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; in and out at an odd dword offset (4 bytes off a 16-byte boundary);
    every output width"""
    name = "frame_shadow"
    pick = np.resize(np.arange(W * H), n)
    cases = [(fn, WIDTHS[fn], family(name, fn)[pick], reference(fn, name)[pick]) for fn in FNS]
    check_ragged(renderer, raw_call(renderer, "sdf_scene", lead=(ctypes.byref(block(name)),)), cases, n)


def test_inside_a_stream_capture(renderer):
    """one capture, replayed twice, the second time over the reversed rays in the same buffers; the counted twin refuses the capturing stream"""
    name = "frame_shadow"
    a = ctypes.byref(block(name))
    twin = raw_call(renderer, "sdf_scene", lead=(a,), counts=(ctypes.c_uint * 2)(7, 7))
    pick = np.arange(1024) + 640                        # rows 10 .. 25 of the frame: hits and sky
    check_capture_replay(renderer, partial(raw_call(renderer, "sdf_scene", lead=(a,)), "render"), family(name, "render")[pick],
                         reference("render", name)[pick], 4, refused_twin=partial(twin, "render"))


def _bad_blocks():
    """(what, edit of an SdfScene, the app's text): blocks SBX_APP_SDF_SCENE refuses"""
    def field(name, value):
        return lambda a: setattr(a, name, value)

    def last_is_an_operator(a):
        a.n_instr = 5
        for i, op in enumerate((M.PLANE, M.OBJECT, M.PLANE, M.PLANE, M.ADD)):
            a.program[i].op, a.program[i].rot_axis, a.program[i].material = op, 0, 1
    return [("n_instr 0", field("n_instr", 0), b"sdf scene: n_instr must lie in 1..32"),
            ("n_instr 33", field("n_instr", 33), b"sdf scene: n_instr must lie in 1..32"),
            ("unknown op", lambda a: setattr(a.program[0], "op", 9), b"sdf scene: unknown op"),
            ("march_steps 0", field("march_steps", 0), b"sdf scene: march_steps must lie in 1..512"),
            ("march_steps 513", field("march_steps", 513), b"sdf scene: march_steps must lie in 1..512"),
            ("shadow 2", field("shadow", 2), b"sdf scene: shadow must be 0 or 1"),
            ("last is not an OBJECT", last_is_an_operator, b"sdf scene: the last instruction must be an OBJECT")]


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    name = "frame_shadow"
    a = block(name)
    rays = torch.from_numpy(family(name, "render")[:4].copy()).to(renderer.tdev)
    wide = torch.zeros((4, 9), dtype=torch.float32, device=renderer.tdev)
    out = torch.full((4, 8), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op, ap = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.byref(a)
    assert lib.sbx_sdf_scene_eval(None, b"render", ap, rp, op, 4, s) == -1
    bad_args = [(ctx, None, ap, rp, op, 4, s), (ctx, b"render", ap, None, op, 4, s), (ctx, b"render", ap, rp, None, 4, s),
                (ctx, b"render", None, rp, op, 4, s), (ctx, b"sdf_shadow", None, rp, op, 0, s),
                (ctx, b"sdf_pipe", ap, rp, op, 4, s), (ctx, b"", ap, rp, op, 4, s), (ctx, b"Render", ap, rp, op, 4, s),
                (ctx, b"render", ap, rp, op, (1 << 31) + 1, s)]
    texts = {}
    for what, edit, text in _bad_blocks():
        b = M.as_aux(C.scene_of(name))
        edit(b)
        for n in (4, 0):                                                                   # the block is checked whatever n is
            bad_args.append((ctx, b"render", ctypes.byref(b), rp, op, n, s))
            texts[len(bad_args) - 1] = (what, text)
    check_refusals(renderer, lib.sbx_sdf_scene_eval, lambda args: lib.sbx_debug_sdf_scene_eval(*args[:-1], (ctypes.c_uint * 2)(7, 7), s), bad_args, out)
    for i, (what, text) in texts.items():                                                  # the app's texts
        assert lib.sbx_sdf_scene_eval(*bad_args[i]) == -1 and text in lib.sbx_last_error(ctx), (what, lib.sbx_last_error(ctx))
        with pytest.raises(SbxError) as app:
            renderer.render("sdf_scene", W, H, 0.0, aux=bad_args[i][2]._obj)
        assert text.decode() in str(app.value), what
    launches = renderer.stats()["render_launches"]
    for fn, (win, wout) in WIDTHS.items():
        assert lib.sbx_sdf_scene_eval(ctx, fn.encode(), ap, None, None, 0, s) == 0         # n == 0 touches nothing
        assert renderer.sdf_scene_eval(fn, torch.zeros((0, win)), a).shape == (0, wout)
        assert renderer.sdf_scene_eval_counted(fn, torch.zeros((0, win)), a)[1] == (0, 0)
        assert renderer.sdf_scene_eval(fn, wide[:, :win], a).shape == (4, wout)
    with pytest.raises(SbxError):
        renderer.sdf_scene_eval("sdf_pipe", rays, a)
    assert lib.sbx_debug_sdf_scene_eval(ctx, b"render", ap, rp, op, 4, None, s) == -1      # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    assert differing(renderer.sdf_scene_eval("render", rays, a), reference("render", name)[:4]) == 0
    assert renderer.stats()["render_launches"] == launches, "not a render"


def test_sdf_is_sbx_sdf_eval(renderer):
    for name in ("seeded", "centres", "specials", "frame_plain"):
        x, a = to_dev(family(name, "sdf")), block(name)
        got = renderer.sdf_scene_eval("sdf", x, a).cpu().numpy()
        assert differing(got, renderer.sdf_eval(a, x).cpu().numpy()) == 0, name


@pytest.mark.parametrize("name", list(M.scenes()))
def test_render_over_the_primary_rays_is_the_apps_frame(renderer, name):
    """"render" over a frame's primary rays, then the model's sRGB step: SBX_APP_SDF_SCENE's frame, which is the fixture's"""
    S = M.scenes()[name]
    a = M.as_aux(S)
    out = renderer.sdf_scene_eval("render", to_dev(E.primary_rays(S, W, H)), a).cpu().numpy()
    frame = renderer.render("sdf_scene", W, H, 0.0, aux=a).cpu().numpy()
    assert_same(E.finish(out[:, :3]).reshape(H, W, 4), frame, name)
    assert_same(frame, M.fixture(name)["frame"], (name, "fixture"))


@pytest.mark.parametrize("name", ["frame_shadow", "frame_plain", "frame_ramp", "seeded", "centres"])
def test_render_impl_is_the_chain_on_the_device(renderer, name):
    """the device's own outputs fed one into the next at "render_impl"'s hit points: sdf_normal -> sdf_ao -> sdf_shadow(p + sun * .05,
    sun) under the block's switch -> illuminate = render_impl's rgb.  The hit point is ray.origin + ray.direction * t, which the march
    computed in the same operations"""
    S, a = C.scene_of(name), block(name)
    run = lambda fn, x: renderer.sdf_scene_eval(fn, to_dev(x), a).cpu().numpy()  # noqa: E731
    rays = family(name, "render_impl")
    impl = run("render_impl", rays)
    hit = impl[:, 4] >= 0
    assert int(hit.sum()) >= 2
    rays, impl = rays[hit], impl[hit]
    p = (rays[:, :3] + rays[:, 3:] * impl[:, 3:4]).astype(F)
    nrm = run("sdf_normal", p)
    ao = run("sdf_ao", np.concatenate([p, nrm], axis=1))
    sh = run("sdf_shadow", C.shadow_rays(S, p)) if S["shadow"] else np.ones_like(ao)
    lit = run("illuminate", np.concatenate([p, nrm, impl[:, 4:5], ao, sh], axis=1))
    assert differing(lit, impl[:, :3]) == 0, name
