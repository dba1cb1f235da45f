"""GPU tests of sbx_egg_eval (include/sbx.h): src/IK.h's solver and APP_EGG's field, normal, shadow march and trace
over the caller's elements under the caller's pose, bit for bit (NaN == NaN) against tests/egg_pose_model.py: the rays of a frame,
seeded points and rays in a box, points on the members' axes (where the witness records and the wave re-runs: both kinds of wave
are counted), a family of NaN / inf / zero / huge values, an untame pose, ragged sizes with guard words, variant 1, a stream capture,
the refusals, "render_scene" tied to SBX_APP_EGG_POSE's frame, and host/sbx_render's --egg-view."""
import ctypes
from functools import partial

import numpy as np
import pytest

from shaderbox_amd import Renderer
from tests import egg_pose_model as M
from tests.app_checks import assert_same, frame_cache, run_sbx_render
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.eval_checks import check_capture_replay, check_ragged, check_refusals, differing, raw_call, to_dev
from tests.model_common import F

pytestmark = pytest.mark.gpu
W, H = M.SIZE
WIDTHS = Renderer.EVAL_WIDTHS["egg"]
FNS = ("sdf", "sdf_normal", "shadowmarch", "render_scene")


def frame_rays(P, w, h):
    fx = (np.arange(w, dtype=F) + F(.5))[None, :]
    fy = (np.arange(h, dtype=F) + F(.5))[:, None]
    pcx, ro, rd = M.primary_rays(P, w, h, fx, fy)
    n = rd[0].size
    return pcx, np.stack([np.full(n, ro[0]), np.full(n, ro[1]), np.full(n, ro[2]), rd[0], rd[1], rd[2]], axis=1).astype(F)


def family(name, win):
    """inputs [n, win] of a family; the pose they are meant for is POSE_OF[name]"""
    rng = np.random.default_rng({"frame": 1, "box": 2, "axes": 3, "specials": 4}[name])
    if name == "frame":
        rays = frame_rays(M.POSES["stride"], W, H)[1]
        return rays if win == 6 else (rays[:, :3] + rays[:, 3:] * rng.uniform(0, 9, size=(len(rays), 1)).astype(F)).astype(F)
    if name == "box":
        o = rng.uniform(-6, 6, size=(1024, 3)) + [0, 0, 3.5]
        d = rng.normal(size=(1024, 3)) * rng.uniform(.2, 2.5, size=(1024, 1))
        return (o if win == 3 else np.concatenate([o, d], axis=1)).astype(F)
    if name == "axes":
        # pose `bones` (turn 0: p = P - (0, .5, 3.5)): the egg's three centres, the wheel's axis, the ring's circle, the feet; as rays:
        # standing there (a zero direction) or running along the axis
        pts = [[0, 1.15, 3.5], [0, .7, 3.5], [0, 1.6, 3.5], [0, -.7, 3.5], [0, -.7, 3.2], [0, -.7, 4.], [1, -.7, 3.5], [0, .3, 3.5],
               [-.3, -.8, 3.3], [.3, -.6, 3.7], [0, .5, 3.3], [0, .5, 3.7]]
        pts = np.array(pts * 6, dtype=F)[:64]
        if win == 3:
            return pts
        d = np.zeros_like(pts)
        d[1::2] = (0, 0, 1)
        return np.concatenate([pts, d], axis=1).astype(F)
    big, nan, inf = 3e38, np.nan, np.inf
    rows = [[0, 0, 0, 0, 0, 0], [0, 1, 8, 0, 0, 0], [0, 1, 8, nan, 0, -1], [0, 1, 8, 0, nan, -1], [nan, 1, 8, 0, 0, -1], [0, 1, 8, inf, 0, -1],
            [0, 1, 8, 0, -inf, 0], [inf, 1, 8, 0, 0, -1], [0, -inf, 8, 0, 0, -1], [0, inf, 8, 0, -1, 0], [big, 1, 8, 0, 0, -1], [0, 1, 8, big, 0, -big],
            [0, 1, 8, 0, 0, -1e-40], [0, 1, 8, 0, 0, -2e4], [2e4, 1, 8, -1, 0, 0], [0, 5e6, 3.5, 0, -1, 0], [0, 1e19, 3.5, 0, -1, 0],
            [0, 1, 8, 0, 0, -1], [0, 9999, 3.5, 0, -9999, 0], [-0., 1, 8, -0., -0., -1]]
    x = np.array(rows, dtype=F)
    return x if win == 6 else x[:, :3].copy()


POSE_OF = {"frame": "stride", "box": "stride", "axes": "bones", "specials": "bones"}


def model(fn, P, x):
    """the model over elements x[n, win] -> [n, wout]"""
    S = M.scene_of(P)
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        if fn == "ik_solver":
            return np.stack(M.ik_solver(tuple(x[:, k] for k in range(3)), tuple(x[:, k] for k in range(3, 6)), x[:, 6], x[:, 7]), axis=1).astype(F)
        if fn == "sdf":
            return np.stack(M.sdf(S, x[:, 0], x[:, 1], x[:, 2]), axis=1).astype(F)
        if fn == "sdf_normal":
            return M.sdf_normal(S, x[:, 0], x[:, 1], x[:, 2])
        o, d = tuple(x[:, k] for k in range(3)), tuple(x[:, k] for k in range(3, 6))
        if fn == "shadowmarch":
            return M.shadowmarch(S, o, d)[:, None]
        rgb, depth = M.render_scene(S, o, d)
        return np.concatenate([rgb, depth[:, None]], axis=1).astype(F)


reference = frame_cache(lambda fn, name: model(fn, M.POSES[POSE_OF[name]], family(name, WIDTHS[fn][0])))


@pytest.mark.parametrize("fn", FNS)
@pytest.mark.parametrize("name", ["frame", "box", "axes", "specials"])
def test_against_the_model(renderer, fn, name):
    x, a = family(name, WIDTHS[fn][0]), M.as_aux(M.POSES[POSE_OF[name]])
    want = reference(fn, name)
    assert want.shape == (len(x), WIDTHS[fn][1])
    assert differing(renderer.egg_eval(fn, to_dev(x), a), want) == 0, (fn, name)
    out, (witnessed, rerun) = renderer.egg_eval_counted(fn, to_dev(x), a)
    assert differing(out, want) == 0, (fn, name, "counted")
    waves = (len(x) + 63) // 64
    print(fn, name, "waves", waves, "witnessed", witnessed, "re-run", rerun)
    if name == "axes":
        assert rerun == waves and witnessed == 0, (fn, "on the members' axes the witness records", witnessed, rerun)
    elif name == "specials":
        assert witnessed == rerun == 0, (fn, "a wave with an untame element takes the plain form", witnessed, rerun)
    else:
        assert witnessed + rerun == waves and witnessed >= waves * 3 // 4, (fn, name, witnessed, rerun)


def test_both_kinds_of_wave_in_one_launch(renderer):
    """64 seeded points, then the 64 on the axes: one wave of each kind, the same bits as apart"""
    P = M.POSES["bones"]
    x = np.concatenate([family("box", 3)[:64], family("axes", 3)], axis=0)
    out, counts = renderer.egg_eval_counted("sdf", to_dev(x), M.as_aux(P))
    assert counts == (1, 1), counts
    assert differing(out, model("sdf", P, x)) == 0


def test_an_untame_pose_takes_the_plain_form(renderer):
    """`reach` (a NaN knee) and a pose with an inf foot: no wave is witnessed or culled, the bits are the model's"""
    x = family("box", 6)[:256]
    for P in (M.POSES["reach"], M.pose((np.inf, 1.3, .2), (-.3, 1.1, -.2)), M.pose((.3, 1.3, .2), (-.3, 1.1, -.2), femur=np.nan)):
        for fn in ("sdf", "render_scene"):
            xi = x[:, :WIDTHS[fn][0]].copy()
            out, counts = renderer.egg_eval_counted(fn, to_dev(xi), M.as_aux(P))
            assert counts == (0, 0), (fn, counts)
            assert differing(out, model(fn, P, xi)) == 0, fn


def test_the_camera_of_the_pose_is_not_read(renderer):
    x = family("box", 6)[:128]
    P = dict(M.POSES["stride"])
    want = renderer.egg_eval("render_scene", to_dev(x), M.as_aux(P)).cpu().numpy()
    P.update(eye=(F(np.nan),) * 3, look_at=(F(np.inf),) * 3, fov=F(-3e38))
    out, counts = renderer.egg_eval_counted("render_scene", to_dev(x), M.as_aux(P))
    assert differing(out, want) == 0 and counts[0] + counts[1] == 2


def test_variant_1_same_bits(renderer, variant_restored):
    for fn in FNS:
        for name in ("frame", "axes", "specials"):
            x, a = family(name, WIDTHS[fn][0]), M.as_aux(M.POSES[POSE_OF[name]])
            for variant in (1, 2, 3):
                renderer.set_variant(variant)
                out, counts = renderer.egg_eval_counted(fn, to_dev(x), a)
                assert differing(out, reference(fn, name)) == 0, (fn, name, variant)
                if variant != 2:
                    assert counts == (0, 0), (fn, name, variant, counts)
            renderer.set_variant(0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_ragged_sizes_bounds_and_alignment(renderer, n):
    """out inside a poisoned buffer with guard words either side; in and out 4 bytes off a 16-byte boundary; every output width"""
    a = M.as_aux(M.POSES["stride"])
    cases = []
    for fn in FNS + ("ik_solver",):
        base = ik_inputs() if fn == "ik_solver" else family("frame", WIDTHS[fn][0])
        full = ik_reference() if fn == "ik_solver" else reference(fn, "frame")
        pick = np.resize(np.arange(len(base)), n)
        cases.append((fn, WIDTHS[fn], base[pick], full[pick]))
    check_ragged(renderer, raw_call(renderer, "egg", lead=(ctypes.byref(a),)), cases, n)


def test_inside_a_stream_capture(renderer):
    """one capture of "render_scene" and of "ik_solver" without a pose, replayed twice, the second time over other elements in the same
    buffers; the counted twin refuses the capturing stream"""
    a = ctypes.byref(M.as_aux(M.POSES["stride"]))
    twin = raw_call(renderer, "egg", lead=(a,), counts=(ctypes.c_uint * 2)(7, 7))
    check_capture_replay(renderer, partial(raw_call(renderer, "egg", lead=(a,)), "render_scene"), family("frame", 6)[:1024],
                         reference("render_scene", "frame")[:1024], 4, refused_twin=partial(twin, "sdf"),
                         also=[(partial(raw_call(renderer, "egg", lead=(None,)), "ik_solver"), ik_inputs()[:256], ik_reference()[:256], 3)])


def test_arguments(renderer):
    import torch
    from shaderbox_amd import SbxError
    lib, ctx, s = renderer.lib, renderer.ctx, renderer._stream()
    a = M.as_aux(M.POSES["stride"])
    rays = torch.from_numpy(family("frame", 6)[:4].copy()).to(renderer.tdev)
    out = torch.full((4, 4), -1.0, dtype=torch.float32, device=renderer.tdev)
    rp, op, ap = ctypes.c_void_p(rays.data_ptr()), ctypes.c_void_p(out.data_ptr()), ctypes.byref(a)
    assert lib.sbx_egg_eval(None, b"render_scene", ap, rp, op, 4, s) == -1
    bad_args = [(ctx, None, ap, rp, op, 4, s), (ctx, b"render_scene", ap, None, op, 4, s), (ctx, b"render_scene", ap, rp, None, 4, s),
                (ctx, b"render_scene", None, rp, op, 4, s), (ctx, b"sdf", None, rp, op, 4, s), (ctx, b"sdf_normal", None, rp, op, 4, s),
                (ctx, b"shadowmarch", None, rp, op, 4, s), (ctx, b"render", ap, rp, op, 4, s), (ctx, b"", ap, rp, op, 4, s),
                (ctx, b"Sdf", ap, rp, op, 4, s), (ctx, b"ik_solver", None, None, op, 1, s), (ctx, b"ik_solver", None, rp, None, 1, s),
                (ctx, b"render_scene", ap, rp, op, (1 << 31) + 1, s), (ctx, b"ik_solver", None, rp, op, (1 << 31) + 1, s)]
    check_refusals(renderer, lib.sbx_egg_eval, lambda args: lib.sbx_debug_egg_eval(*args[:-1], (ctypes.c_uint * 2)(7, 7), s), bad_args, out)
    for fn, (win, wout) in WIDTHS.items():
        assert lib.sbx_egg_eval(ctx, fn.encode(), ap, None, None, 0, s) == 0            # n == 0 touches nothing
        assert renderer.egg_eval(fn, torch.zeros((0, win)), a).shape == (0, wout)
    with pytest.raises(SbxError):
        renderer.egg_eval("render", rays, a)
    assert lib.sbx_debug_egg_eval(ctx, b"render_scene", ap, rp, op, 4, None, s) == -1    # the hook needs a place for its counts
    torch.cuda.synchronize()
    assert bool((out == -1.0).all())
    before = renderer.stats()["render_launches"]                                         # not a render
    assert differing(renderer.egg_eval("render_scene", rays, a), reference("render_scene", "frame")[:4]) == 0
    assert renderer.stats()["render_launches"] == before


@pytest.mark.parametrize("name", ["stride", "inside"])
def test_render_scene_over_the_primary_rays_is_the_apps_frame(renderer, name):
    """"render_scene" over a frame's primary rays, then render's bars, abs and sRGB from the model: SBX_APP_EGG_POSE's frame"""
    P = M.POSES[name]
    pcx, rays = frame_rays(P, W, H)
    out = renderer.egg_eval("render_scene", to_dev(rays), M.as_aux(P)).cpu().numpy()
    frame = renderer.render("egg_pose", W, H, 0.0, aux=M.as_aux(P)).cpu().numpy()
    assert_same(M.finish(out[:, :3], out[:, 3], pcx).reshape(H, W, 4), frame, name)
    assert_same(frame, M.fixture(name)["frame"], (name, "fixture"))


# ---- "ik_solver" ---------------------------------------------------------------------------------------------------------------------

def ik_inputs():
    """4096 seeded elements: reachable goals, unreachable ones, folded ones (inside |L1 - L2|), goal = start, zero bones, G = L1 + L2
    exactly, goals off the start's z plane, and non-finite values"""
    rng = np.random.default_rng(5)
    n = 4096
    start = rng.uniform(-1, 1, size=(n, 3))
    l1, l2 = rng.uniform(.2, 1.2, size=n), rng.uniform(.2, 1.2, size=n)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    reach = rng.uniform(0, 1.4, size=n) * (l1 + l2)                       # beyond 1: unreachable; below |l1 - l2|: folded
    x = np.concatenate([start, start + d * reach[:, None], l1[:, None], l2[:, None]], axis=1).astype(F)
    x[0:32, 3:6] = x[0:32, 0:3]                                           # goal = start
    x[32:48, 6] = 0                                                       # L1 = 0
    x[48:64, 7] = 0                                                       # L2 = 0
    x[64:96, 0:3] = 0                                                     # zero start
    x[96:112, 3:6] = 0                                                    # zero goal
    x[112:128] = np.array([0, 0, 0, 0, 1.5, 0, 1, .5], dtype=F)           # G = L1 + L2 exactly
    x[128:136, 3] = np.nan
    x[136:144, 4] = np.inf
    x[144:152, 6] = np.inf
    x[152:160, 7] = np.nan
    x[160:168, 0] = -np.inf
    return x


ik_reference = frame_cache(lambda: model("ik_solver", M.POSES["stride"], ik_inputs()))


def test_ik_solver_seeded_goals(renderer):
    x, want = ik_inputs(), ik_reference()
    reach = np.linalg.norm(x[:, 3:6].astype(np.float64) - x[:, :3], axis=1)
    assert (reach > x[:, 6] + x[:, 7]).sum() > 500 and (reach < np.abs(x[:, 6] - x[:, 7])).sum() > 100, "unreachable and folded goals are there"
    assert 500 < int(np.isnan(want).any(axis=1).sum()) < 3000
    assert differing(renderer.egg_eval("ik_solver", to_dev(x)), want) == 0
    assert differing(renderer.egg_eval("ik_solver", to_dev(x), M.as_aux(M.POSES["reach"])), want) == 0       # a pose changes nothing


def test_ik_solver_gives_the_knees_of_the_default_pose(renderer):
    """the two knees build_egg computes on the host (and hands to k_egg in the frame block), through the model's scene"""
    for t in (0.0, 1.3, 7.77):
        P = M.default_pose(t)
        S = M.scene_of(P)
        x = np.array([list(S["pelvis_l"]) + list(P["left_foot"]) + [P["femur"], P["tibia"]],
                      list(S["pelvis_r"]) + list(P["right_foot"]) + [P["femur"], P["tibia"]]], dtype=F)
        want = np.array([S["knee_l"], S["knee_r"]], dtype=F)
        assert np.isfinite(want).all()
        assert differing(renderer.egg_eval("ik_solver", to_dev(x)), want) == 0, t


def test_egg_view_of_sbx_render(renderer, tmp_path):
    """host/sbx_render --egg-view with the stride pose's camera and pose flags writes that fixture; with the shipped camera and no
    flags, SBX_APP_EGG's frame of --time"""
    P = M.POSES["stride"]
    c = lambda v: ",".join(repr(float(x)) for x in v)  # noqa: E731
    view = ["--egg-view", str(W), str(H)] + [repr(float(v)) for v in P["eye"]] + [repr(float(v)) for v in P["look_at"]]
    flags = view + ["--fov", repr(float(P["fov"])), "--turn", repr(float(P["turn_deg"])), "--left-foot", c(P["left_foot"]),
                    "--right-foot", c(P["right_foot"])]
    assert_same(run_sbx_render(tmp_path, "egg", W, H, 0.0, flags=flags), M.fixture("stride")["frame"], "--egg-view, stride")
    shipped = ["--egg-view", str(W), str(H), "0", "0.25", "5.25", "0", "0.25", "0"]
    assert_same(run_sbx_render(tmp_path, "egg", W, H, 1.3, flags=shipped), renderer.render("egg", W, H, 1.3).cpu().numpy(), "--egg-view, shipped")
