"""GPU tests of SBX_APP_SDF_SCENE and sbx_sdf_eval (include/sbx.h): k_sdf_scene / k_sdf_scene_eval over the caller's
field, every comparison bit for bit with NaN == NaN against tests/sdf_scene_model.py — the ramp block, seeded and edge scenes, the
field on its own per primitive and per operator — then the layers above the kernel, the refusals and sbx_main_image's cache."""
import numpy as np
import pytest

import shaderbox_amd
from tests import sdf_scene_model as M
from tests.app_checks import (assert_same, check_loopback_exchanges, check_multi_render, check_rgba8, check_rows_host_rows_ranks_and_splits,
                              edge_points, frame_cache, run_sbx_render, same_tensor)
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F

pytestmark = pytest.mark.gpu

APP = "sdf_scene"
SIZES = [(64, 36), (67, 35)]
TIMES = [0.0, 0.37, 2.5]

ramp_frame = frame_cache(lambda t, w, h: M.frame(M.ramp_scene(t), w, h))


# ---- the default block ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
def test_no_block_is_the_ramp_block_is_the_model(renderer, size):
    w, h = size
    for t in TIMES:
        want = ramp_frame(t, w, h)
        assert_same(renderer.render(APP, w, h, t), want, ("aux = None", t))
        a = shaderbox_amd.sdf_ramp_scene(w, h, t)
        assert bytes(a) == M.to_block(M.ramp_scene(t))
        assert_same(renderer.render(APP, w, h, t, aux=a), want, ("the ramp block", t))
        same_tensor(renderer.render(APP, w, h, -9.0, mouse=(3.0, 200.0), aux=a), renderer.render(APP, w, h, t, aux=a), "u_time and u_mouse are not read")


# ---- what the reference's header rendered ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(M.scenes()))
def test_fixture_scenes_are_the_reference(renderer, variant_restored, name):
    import torch
    w, h = M.scene_table()["size"]
    fx, S = M.fixture(name), M.scenes()[name]
    a = M.as_aux(S)
    for variant in (0, 1):
        renderer.set_variant(variant)
        assert_same(renderer.render(APP, w, h, 0.0, aux=a), fx["frame"], (name, "frame", variant))
        assert_same(renderer.render_points(APP, w, h, 0.0, torch.from_numpy(fx["points"]), aux=a), fx["points_out"], (name, "points", variant))
    pts = cloud()
    assert_same(renderer.sdf_eval(a, torch.from_numpy(pts)), eval_model(S, pts), (name, "the field of the full program"))


# ---- seeded tame scenes against the model -----------------------------------------------------------------------------------------

N_INSTR = {0: 2, 1: 32, 2: 4, 5: 32}
STEPS = {3: 1, 4: 512, 5: 512}


def tame(seed):
    return M.tame_scene(seed, N_INSTR.get(seed), STEPS.get(seed, 70))


tame_frame = frame_cache(lambda seed, w, h: M.frame(tame(seed), w, h))


def test_tame_scenes_cover_what_they_should():
    """(an object of k primitives takes 2k instructions, so a program's length is even: 2 is the shortest)"""
    scenes = [tame(s) for s in range(20)]
    assert {len(S["program"]) for S in scenes} >= {2, 4, 32}
    assert max(M.depth_of(S) for S in scenes) == M.MAX_STACK
    ops = {I["op"] for S in scenes for I in S["program"]}
    assert ops == set(M.PRIMITIVES + M.OPERATORS + (M.OBJECT,))
    assert {I["rot_axis"] for S in scenes for I in S["program"] if I["op"] in M.PRIMITIVES} == {0, 1, 2, 3}
    assert {S["march_steps"] for S in scenes} == {1, 70, 512} and {S["shadow"] for S in scenes} == {0, 1}


@pytest.mark.parametrize("seed", range(20))
def test_seeded_tame_scenes_are_the_model(renderer, seed):
    w, h = SIZES[seed % 2]
    S = tame(seed)
    assert_same(renderer.render(APP, w, h, 0.0, aux=M.as_aux(S)), tame_frame(seed, w, h), ("tame scene", seed, len(S["program"])))


@pytest.mark.parametrize("seed", [1, 6, 15])
def test_default_witness_edge_and_ieee_kernels_agree(renderer, variant_restored, seed):
    w, h = SIZES[seed % 2]
    a, want = M.as_aux(tame(seed)), tame_frame(seed, w, h)
    for v in (0, 1, 2):
        renderer.set_variant(v)
        assert_same(renderer.render(APP, w, h, 0.0, aux=a), want, ("variant", v, seed))


# ---- the field on its own ---------------------------------------------------------------------------------------------------------

def cloud():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-3, 3, (1500, 3)).astype(F)
    e = np.array([0.0, -0.0, 1e-40, -1e-40, 1e30, -1e30, np.inf, -np.inf, np.nan, 1.0], dtype=F)
    edge = np.stack(np.meshgrid(e, e, e, indexing="ij"), axis=-1).reshape(-1, 3)
    on_axis = np.array([[0, 0, 0], [0, 1, 0], [.5, 0, 0], [0, 0, .5]], dtype=F)      # a root of exactly 0: the witness records it
    return np.concatenate([pts, edge, on_axis]).astype(F)


def eval_model(S, pts):
    d, m = M.sdf(S, pts[:, 0], pts[:, 1], pts[:, 2])
    return np.stack([d, m], axis=1).astype(F)


def one_primitive(kind, seed, rotated):
    rng = np.random.default_rng(100 * kind + seed)
    I = M.random_primitive(rng, kind)
    if not rotated:
        I["rot_axis"] = 0
    return I


def program_scene(P):
    return dict(M.ramp_scene(0.0), program=P)


@pytest.mark.parametrize("kind", M.PRIMITIVES)
def test_sdf_eval_per_primitive(renderer, variant_restored, kind):
    import torch
    pts = cloud()
    assert len(pts) <= 4096
    for seed, axis in enumerate((0, 1, 2, 3)):
        I = one_primitive(kind, seed, axis != 0)
        I["rot_axis"] = axis
        S = program_scene([I, M.obj(seed)])
        want = eval_model(S, pts)
        for v in (0, 1, 2):
            renderer.set_variant(v)
            assert_same(renderer.sdf_eval(M.as_aux(S), torch.from_numpy(pts)), want, ("primitive", kind, "axis", axis, "variant", v))


@pytest.mark.parametrize("op", M.OPERATORS)
def test_sdf_eval_per_operator(renderer, op):
    import torch
    pts = cloud()
    for seed, k in enumerate((.3, 0.0, float("inf"), -.2)):
        rng = np.random.default_rng(seed)
        a, b = M.random_primitive(rng, M.BOX), M.random_primitive(rng, M.SPHERE)
        b["offset"] = a["offset"]
        S = program_scene([M.instr(M.PLANE, a=(0, 1, 0, 0)), M.obj(7), a, b, M.instr(op, a=(k,)), M.obj(3)])
        assert_same(renderer.sdf_eval(M.as_aux(S), torch.from_numpy(pts)), eval_model(S, pts), ("operator", op, "k", k))


def test_sdf_eval_of_full_programs(renderer):
    import torch
    pts = cloud()
    for S in [M.ramp_scene(0.37)] + [tame(s) for s in (1, 5, 8, 13)] + [edge_scene("geometry")]:
        assert_same(renderer.sdf_eval(M.as_aux(S), torch.from_numpy(pts)), eval_model(S, pts), ("program of", len(S["program"])))


def test_sdf_eval_reads_only_the_program_and_no_points_touch_nothing(renderer):
    import torch
    pts = cloud()[:256]
    S = tame(8)
    want = eval_model(S, pts)
    a = M.as_aux(S)
    a.march_steps, a.shadow, a.view, a.checker_material, a.march_end = 0, 9, -3, 99, float("nan")
    assert_same(renderer.sdf_eval(a, torch.from_numpy(pts)), want, "the renderer's settings are not read")
    out = torch.full((16, 2), -7.0, dtype=torch.float32, device=renderer.tdev)
    xyz = torch.zeros((16, 3), dtype=torch.float32, device=renderer.tdev)
    rc = renderer.lib.sbx_sdf_eval(renderer.ctx, a, xyz.data_ptr(), out.data_ptr(), 0, None)
    torch.cuda.synchronize()
    assert rc == shaderbox_amd.SBX_OK and bool((out == -7.0).all())
    launches = renderer.stats()["render_launches"]
    renderer.sdf_eval(a, torch.from_numpy(pts))
    assert renderer.stats()["render_launches"] == launches, "not counted in render_launches"


# ---- numbers that are no scene ----------------------------------------------------------------------------------------------------

def edge_scene(kind):
    """Objects whose value is a NaN everywhere — a zero-length cylinder and capsule, a collinear Bezier, rot_deg inf, a NaN plane normal,
    an inf offset under a rotation — each replaced by the object after it (`acc.x < v.x` is false against a NaN); then a plane far below,
    a sphere of radius 0, blends with k = 0 and k = inf (the latter -inf everywhere, cut back to its box by INTERSECT), a box at offset
    1e30 with half-width 1e30 (|pos.x - 1e30| - 1e30 is 0), and last max(5 y, -1): a plane whose normal has length 5, so the march
    oversteps it, cut by a plane of normal 0 and distance -1 — below y = -.2 the field is the constant -1, a hit whose six taps are
    equal: normalize(0, 0, 0), NaN pixels for the rays that go down, none for those that go up.
    "nan_end": march_end NaN (`t > end` never holds); "fov0": fov 0 (every pixel the one ray to look_at)."""
    inf, nan = float("inf"), float("nan")
    P = [M.instr(M.CYLINDER, (0, 1, 0), (.2, .2, .2, .1), (.2, .2, .2)), M.obj(2),
         M.instr(M.CAPSULE, (1, 1, 0), (.1, .2, .3, .1), (.1, .2, .3)), M.obj(3),
         M.instr(M.BEZIER, (0, 1, 1), (-1, 0, 0, .1), (0, 0, 0), (1, 0, 0)), M.obj(4),
         M.instr(M.SPHERE, (0, 1, 0), (.5,), rot_axis=2, rot_deg=inf), M.obj(5),
         M.instr(M.PLANE, (0, 0, 0), (nan, 1, 0, 0)), M.obj(6),
         M.instr(M.BOX, (inf, 0, 0), (1, 1, 1), rot_axis=3, rot_deg=30.0), M.obj(7),
         M.instr(M.PLANE, (0, 0, 0), (0, 1, 0, 5)), M.obj(1),
         M.instr(M.SPHERE, (1.5, 1, 0), (0.0,)), M.obj(2),
         M.instr(M.BOX, (-1.5, .5, 0), (.5, .5, .5)), M.instr(M.SPHERE, (-1.5, 1.1, 0), (.5,)), M.instr(M.BLEND, a=(0.0,)), M.obj(3),
         M.instr(M.BOX, (0, .4, -1.5), (.4, .4, .4)), M.instr(M.SPHERE, (0, .4, -1.5), (.5,)), M.instr(M.Y_CYLINDER, (0, .4, -1.5), (.2, 2)),
         M.instr(M.BLEND, a=(inf,)), M.instr(M.INTERSECT), M.obj(4),
         M.instr(M.BOX, (1e30, .5, 1.5), (1e30, .25, .25)), M.obj(5),
         M.instr(M.PLANE, (0, 0, 0), (0, 5, 0, 0)), M.instr(M.PLANE, (0, 0, 0), (0, 0, 0, -1)), M.instr(M.INTERSECT), M.obj(6)]
    S = dict(M.ramp_scene(0.37), program=P, shadow=1)
    if kind == "nan_end":
        S["march_end"] = F(nan)
    elif kind == "fov0":
        S["fov"] = F(0)
    assert M.check(S) is None
    return S


edge_frame = frame_cache(lambda kind, w, h: M.frame(edge_scene(kind), w, h))


@pytest.mark.parametrize("kind", ["geometry", "nan_end", "fov0"])
def test_edge_scenes_are_the_model(renderer, variant_restored, kind):
    w, h = SIZES[1]
    a, want = M.as_aux(edge_scene(kind)), edge_frame(kind, w, h)
    nans = int(np.isnan(want[..., :3]).any(axis=-1).sum())
    for v in (0, 1):
        renderer.set_variant(v)
        got = renderer.render(APP, w, h, 0.0, aux=a).cpu().numpy()
        assert_same(got, want, ("edge scene", kind, "variant", v))
        assert int(np.isnan(got[..., :3]).any(axis=-1).sum()) == nans and (got[..., 3] == 1).all()
    if kind == "fov0":
        assert (want.view(np.uint32) == want.view(np.uint32)[0, 0]).all(), "one ray"
    else:
        assert 0 < nans < w * h, "the rays that go down end in the constant field, the others do not"


def test_edge_points_are_the_model(renderer):
    import torch
    w, h = SIZES[0]
    pts = edge_points(w, h)
    S = tame(7)
    assert_same(renderer.render_points(APP, w, h, 0.0, torch.from_numpy(pts), aux=M.as_aux(S)), M.points(S, w, h, pts), "edge points")


# ---- the layers above the kernel --------------------------------------------------------------------------------------------------

def test_rows_host_rows_ranks_and_splits(renderer):
    w, h = SIZES[1]
    check_rows_host_rows_ranks_and_splits(renderer, APP, w, h, 0.0, tame_frame(9, w, h), cuts=[13, 14, 30], block_rows=8, aux=M.as_aux(tame(9)))


def test_rgba8_frames(renderer):
    w, h = SIZES[1]
    assert_same(check_rgba8(renderer, APP, w, h, 0.0, aux=M.as_aux(tame(11))), tame_frame(11, w, h), "the float frame")


def test_main_image_pixel_and_point(renderer):
    w, h = SIZES[0]
    S = tame(10)
    a, want = M.as_aux(S), tame_frame(10, w, h)
    for x, y in [(0, 0), (40, 17), (63, 35)]:
        assert_same(np.array(renderer.main_image(APP, w, h, 0.0, (x + .5, y + .5), aux=a), dtype=F), want[y, x], ("pixel", x, y))
    pt = np.array([[40.25, 17.75]], dtype=F)
    assert_same(np.array(renderer.main_image(APP, w, h, 0.0, tuple(pt[0]), aux=a), dtype=F), M.points(S, w, h, pt)[0], "off-centre point")


def test_span_table_is_whole_rows():
    w, h = 256, 144
    for aux in (None, M.as_aux(tame(3))):
        table, pix, mw = shaderbox_amd.span_table(APP, w, h, 0.0, 8, 3, aux=aux)
        assert (table[:, 0] == 0).all() and (table[:, 1] == w).all() and mw == w and int(pix.sum()) == w * h


def test_exchanges_through_loopback_ranks(renderer):
    w, h = SIZES[0]
    check_loopback_exchanges(renderer, APP, 2, w, h, 0.37)


def test_multi_render():
    w, h = SIZES[0]
    check_multi_render(APP, w, h, 0.37, lambda: ramp_frame(0.37, w, h))


def test_sbx_render_host_reads_a_scene_file(tmp_path):
    import os
    import subprocess
    w, h = SIZES[1]
    path = tmp_path / "scene.bin"
    path.write_bytes(M.to_block(tame(12)))
    assert_same(run_sbx_render(tmp_path, APP, w, h, 0.0, flags=["--scene-bin", str(path)]), tame_frame(12, w, h), "sbx_render --scene-bin")
    assert_same(run_sbx_render(tmp_path, APP, w, h, 0.37), ramp_frame(0.37, w, h), "sbx_render without a scene file")
    (tmp_path / "short.bin").write_bytes(M.to_block(tame(12))[:-4])
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "host", "sbx_render")
    r = subprocess.run([exe, "--app", APP, "--res", "8x8", "--scene-bin", str(tmp_path / "short.bin")], capture_output=True, timeout=60)
    assert r.returncode == 2, "a file of another size is refused"


def test_captured_launch_replays(renderer):
    import torch
    w, h = SIZES[0]
    a = M.as_aux(tame(14))
    out = torch.zeros((h, w, 4), dtype=torch.float32, device=renderer.tdev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    launches = renderer.stats()["render_launches"]
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            renderer.render(APP, w, h, 0.0, aux=a, out=out)
    assert renderer.stats()["render_launches"] == launches + 1, "one launch"
    a.march_steps = 1                                              # the block was read during the call: the graph holds its own copy
    out.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, tame_frame(14, w, h), "graph replay")


# ---- refusals and the frame cache -------------------------------------------------------------------------------------------------

def _set(field, value):
    return lambda a: setattr(a, field, value)


def _instr(i, field, value):
    return lambda a: setattr(a.program[i], field, value)


def _program(*ops):
    def edit(a):
        a.n_instr = len(ops)
        for i, op in enumerate(ops):
            a.program[i].op, a.program[i].rot_axis, a.program[i].material = op, 0, 1
    return edit


P_, O_, A_ = M.PLANE, M.OBJECT, M.ADD
# (the ramp block: instruction 0 is a BOX, 2 a SUB, 3 and 19 are OBJECTs)
BAD = {"n_instr 0": _set("n_instr", 0), "n_instr 33": _set("n_instr", 33), "n_instr -1": _set("n_instr", -1),
       "op 0": _instr(0, "op", 0), "op 9": _instr(0, "op", 9), "op 15": _instr(0, "op", 15), "op 20": _instr(2, "op", 20), "op 33": _instr(3, "op", 33),
       "op -1": _instr(0, "op", -1), "rot_axis -1": _instr(0, "rot_axis", -1), "rot_axis 4": _instr(0, "rot_axis", 4),
       "material -1": _instr(3, "material", -1), "material 8": _instr(19, "material", 8),
       "underflow at an OBJECT": _program(O_), "underflow at an operator": _program(P_, A_, O_), "overflow": _program(P_, P_, P_, P_, P_, A_, A_, A_, A_, O_),
       "not empty at an OBJECT": _program(P_, P_, O_, P_, O_), "not empty at the end": _program(P_, O_, P_), "last is an operator": _program(P_, O_, P_, P_, A_)}
BAD_RENDER = {"checker -2": _set("checker_material", -2), "checker 8": _set("checker_material", 8), "march_steps 0": _set("march_steps", 0),
              "march_steps 513": _set("march_steps", 513), "shadow -1": _set("shadow", -1), "shadow 2": _set("shadow", 2),
              "view -1": _set("view", -1), "view 2": _set("view", 2)}


@pytest.mark.parametrize("case", list(BAD) + list(BAD_RENDER))
def test_bad_blocks_are_refused_before_anything_is_enqueued(renderer, case):
    import torch
    w, h = SIZES[0]
    a = shaderbox_amd.sdf_ramp_scene(w, h, 0.0)
    assert shaderbox_amd.sdf_scene_check(a) is None
    {**BAD, **BAD_RENDER}[case](a)
    assert shaderbox_amd.sdf_scene_check(a) is not None
    out = torch.full((h, w, 4), -7.0, dtype=torch.float32, device=renderer.tdev)
    launches = renderer.stats()["render_launches"]
    with pytest.raises(shaderbox_amd.SbxError) as e:
        renderer.render(APP, w, h, 0.0, aux=a, out=out)
    assert e.value.code == shaderbox_amd.SBX_ERR_ARG
    if case in BAD:
        pts = torch.zeros((64, 3), dtype=torch.float32, device=renderer.tdev)
        vals = torch.full((64, 2), -7.0, dtype=torch.float32, device=renderer.tdev)
        assert renderer.lib.sbx_sdf_eval(renderer.ctx, a, pts.data_ptr(), vals.data_ptr(), 64, None) == shaderbox_amd.SBX_ERR_ARG
        torch.cuda.synchronize()
        assert bool((vals == -7.0).all())
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and renderer.stats()["render_launches"] == launches


def test_programs_at_the_bounds_are_accepted(renderer):
    w, h = SIZES[0]
    S = tame(1)
    assert len(S["program"]) == 32 and M.depth_of(S) == 4
    S["program"][-1]["material"], S["program"][1]["material"] = 7, 0
    assert_same(renderer.render(APP, w, h, 0.0, aux=M.as_aux(S)), M.frame(S, w, h), "32 instructions, depth 4, materials 0 and 7")


def test_main_image_cache_tells_scene_blocks_apart(renderer):
    """two blocks that differ only in their LAST instruction (byte 2716 of 2784, an OBJECT's material) under the same uniforms: each
    call gets its own block's frame — the cache key holds the whole block (FrameCache::KEY_WORDS)"""
    w, h = SIZES[0]
    Sa = tame(1)
    Sb = dict(Sa, program=[dict(I) for I in Sa["program"]])
    Sb["program"][-1]["material"] = (Sa["program"][-1]["material"] + 1) % 8
    a, b = M.to_block(Sa), M.to_block(Sb)
    assert len(Sa["program"]) == 32 and a[:2704] == b[:2704] and a != b
    fa, fb = M.frame(Sa, w, h), M.frame(Sb, w, h)
    ys, xs = np.nonzero((fa.view(np.uint32) != fb.view(np.uint32)).any(axis=-1))
    assert len(ys) > 0, "the last object is seen"
    y, x = int(ys[0]), int(xs[0])
    for _ in range(2):
        assert_same(np.array(renderer.main_image(APP, w, h, 0.0, (x + .5, y + .5), aux=M.as_aux(Sa)), dtype=F), fa[y, x], "block a")
        assert_same(np.array(renderer.main_image(APP, w, h, 0.0, (x + .5, y + .5), aux=M.as_aux(Sb)), dtype=F), fb[y, x], "block b")
