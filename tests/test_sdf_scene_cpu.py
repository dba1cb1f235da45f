"""CPU tests of SBX_APP_SDF_SCENE's definition (tests/sdf_scene_model.py; include/sbx.h): its renderer over the shipped
sdf is tests/sdf_ao_builds_model.py's frame in every bit, over the scenes of tests/golden/sdf_scenes.json it is what the reference's
own header rendered with those scenes written into it (tools/make_golden_sdf_scenes.py), the blocks' Python layout is the C header's,
the host validator refuses what include/sbx.h lists, and sbx_sdf_scene_ramp is the model's ramp block."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

import shaderbox_amd
from tests import sdf_ao_builds_model as B
from tests import sdf_scene_model as M
from tests.model_common import F, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def differing(a, b):
    return int((~same_bits(a, b)).any(axis=-1).sum())


# ---- the parameterised renderer is app_sdf_ao.h's -----------------------------------------------------------------------------------

@pytest.mark.parametrize("build", B.BUILDS)
def test_renderer_over_the_shipped_sdf_is_the_builds_model(build):
    w, h = 64, 36
    for t in (0.37, 2.5):
        eye, look_at = B.camera(t)
        R = dict(eye=eye, look_at=look_at, fov=B.FOV, march_steps=70, march_end=F(20.), sun_dir=B.sun_dir(), background=(F(.1), F(.1), F(.7)),
                 shadow=int(build == "shadow"), view=int(build == "normals"), checker_material=1, fog_density=B.FOG_DENSITY,
                 fog_falloff=B.FOG_FALLOFF, materials=M.SHIPPED_MATERIALS)
        assert differing(M.render_frame(B.sdf, R, w, h), B.frame(build, w, h, t)) == 0, (build, t)


# ---- the fixtures ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fixture_frames():
    w, h = M.scene_table()["size"]
    frames = {name: M.frame(S, w, h) for name, S in M.scenes().items()}
    masks = {name: M.masks(S, w, h) for name, S in M.scenes().items()}
    return frames, masks


def test_fixtures_are_the_model_and_meet_their_conditions(fixture_frames):
    frames, masks = fixture_frames
    table = M.scene_table()
    (w, h), n = table["size"], table["points"]
    assert (w, h, n) == (64, 36, 64)
    bound = max(os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*.npz")))
    recorded = {}
    for e in table["scenes"]:
        name, S = e["name"], M.scene_of(e)
        fx = M.fixture(name)
        assert set(fx.files) == {"frame", "points", "points_out"}
        assert os.path.getsize(os.path.join(M.GOLDEN, "sdf_scenes", "%s_%dx%d.npz" % (name, w, h))) <= bound
        assert np.array_equal(fx["points"], M.fixture_points(e["points_seed"], w, h, n))
        assert differing(frames[name], fx["frame"]) == 0, (name, "the model is not what the reference's header rendered")
        assert differing(M.points(S, w, h, fx["points"]), fx["points_out"]) == 0, (name, "points")
        recorded[name] = fx["frame"]
    M.check_conditions(table, recorded, masks)


def test_the_table_holds_settings_only():
    def leaves(v):
        if isinstance(v, dict):
            for x in v.values():
                yield from leaves(x)
        elif isinstance(v, list):
            for x in v:
                yield from leaves(x)
        else:
            yield v
    for e in M.scene_table()["scenes"]:
        assert e["name"].isidentifier() and M.entry_of(e["name"], e["points_seed"], M.scene_of(e)) == e
        for key, v in e.items():
            for leaf in leaves(v):
                if isinstance(leaf, str) and key != "name" and leaf not in M.OP_VALUES:
                    assert np.isfinite(float.fromhex(leaf)) and F(float.fromhex(leaf)) == float.fromhex(leaf), (e["name"], key, leaf)
                else:
                    assert isinstance(leaf, (int, str))


# ---- the blocks -----------------------------------------------------------------------------------------------------------------------

LAYOUT = r'''
#include "sbx.h"
#include <cstdio>
#define O(f) (int)offsetof(sbx_aux_sdf_scene, f)
#define I(f) (int)offsetof(sbx_sdf_instr, f)
int main() { printf("%d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d\n",
    (int)sizeof(sbx_aux_sdf_scene), (int)sizeof(sbx_sdf_instr),
    O(eye), O(fov), O(look_at), O(march_steps), O(sun_dir), O(march_end), O(background), O(shadow), O(fog_density), O(fog_falloff), O(view),
    O(checker_material), O(n_instr), O(materials), O(program),
    I(op), I(rot_axis), I(rot_deg), I(material), I(offset), I(a), I(b), I(c),
    SBX_SDF_PLANE, SBX_SDF_SPHERE, SBX_SDF_BOX, SBX_SDF_TORUS, SBX_SDF_Y_CYLINDER, SBX_SDF_CYLINDER, SBX_SDF_CAPSULE, SBX_SDF_BEZIER,
    SBX_SDF_ADD, SBX_SDF_SUB, SBX_SDF_INTERSECT, SBX_SDF_BLEND, SBX_SDF_OBJECT, SBX_SDF_MAX_INSTR, SBX_SDF_MAX_STACK);
    return SBX_APP_SDF_SCENE == 33 && SBX_ABI_VERSION == 2 ? 0 : 1; }
'''


def test_ctypes_layout_is_the_headers(tmp_path):
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text(LAYOUT)
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A, In, s = shaderbox_amd.SdfScene, shaderbox_amd.SdfInstr, shaderbox_amd
    want = [ctypes.sizeof(A), ctypes.sizeof(In)]
    want += [getattr(A, f).offset for f in ("eye", "fov", "look_at", "march_steps", "sun_dir", "march_end", "background", "shadow", "fog_density",
                                            "fog_falloff", "view", "checker_material", "n_instr", "materials", "program")]
    want += [getattr(In, f).offset for f in ("op", "rot_axis", "rot_deg", "material", "offset", "a", "b", "c")]
    want += [s.SDF_PLANE, s.SDF_SPHERE, s.SDF_BOX, s.SDF_TORUS, s.SDF_Y_CYLINDER, s.SDF_CYLINDER, s.SDF_CAPSULE, s.SDF_BEZIER, s.SDF_ADD, s.SDF_SUB,
             s.SDF_INTERSECT, s.SDF_BLEND, s.SDF_OBJECT, s.SDF_MAX_INSTR, s.SDF_MAX_STACK]
    assert got == want and got[:2] == [2784, 80] == [M.BLOCK_BYTES, M.INSTR_BYTES]
    assert (M.PRIMITIVES, M.OPERATORS, M.OBJECT) == (tuple(range(s.SDF_PLANE, s.SDF_BEZIER + 1)), tuple(range(s.SDF_ADD, s.SDF_BLEND + 1)), s.SDF_OBJECT)
    assert s.app_id("sdf_scene") == s.APP_SDF_SCENE == 33 == s.ALL_APPS["APP_SDF_SCENE"]


def test_blocks_round_trip():
    for S in list(M.scenes().values()) + [M.tame_scene(s) for s in range(4)]:
        b = M.to_block(S)
        assert M.to_block(M.from_block(b)) == b and bytes(M.as_aux(S)) == b
        assert shaderbox_amd.sdf_scene_check(M.as_aux(S)) is None and M.check(S) is None


@pytest.mark.parametrize("t", [0.0, 0.37, 2.5, -7.25, 1e9])
def test_ramp_block_of_the_library_is_the_models(t):
    a = shaderbox_amd.sdf_ramp_scene(64, 36, t)
    assert bytes(a) == M.to_block(M.ramp_scene(t))
    assert a.n_instr == 20 and M.depth_of(M.from_block(a)) == 4 and shaderbox_amd.sdf_scene_check(a) is None
    assert bytes(shaderbox_amd.sdf_ramp_scene(1920, 1080, t)) == bytes(a), "u_res does not enter the block"


def test_builder_states_the_ramp_block():
    b = shaderbox_amd.SdfSceneBuilder()
    sx, sy, sz = F(1.3), F(1.), F(1.25)
    o1, o2, H = (0, sy, 0), (0, sy * F(2), 0), F(-.125)
    b.box(o1, (sx, sy, sz)).y_cylinder((F(0) + F(.7), sy + F(.5), 0), sy + F(.55), F(2) * sz + F(.1), rot_axis=1, rot_deg=-90).sub().object(2)
    b.y_cylinder((F(0) + (-sx + F(.525)), sy + sy, 0), F(.025), F(2) * sz, rot_axis=1, rot_deg=-90).object(5)
    b.box((F(0) - sx, o2[1] - F(-.25), 0), (F(.025), F(.05), sz))
    bar = lambda z: b.box((F(0) - sx, o2[1] - H, F(0) - z), (F(.025), F(.125), F(.025)))  # noqa: E731
    bar(F(0)), bar(sz / F(2))
    b.add()
    bar(sz)
    b.add()
    bar(-sz / F(2)), bar(-sz)
    b.add().add().add().object(4).plane((0, 1, 0), 0).object(1)
    want = shaderbox_amd.sdf_ramp_scene(64, 36, 0.0)
    got = b.set(eye=list(want.eye), sun_dir=list(want.sun_dir)).scene()
    assert bytes(got) == bytes(want)


# ---- the host validator ---------------------------------------------------------------------------------------------------------------

def test_validator_refuses_what_the_header_lists():
    from tests.test_gpu_sdf_scene import BAD, BAD_RENDER
    for case, edit in {**BAD, **BAD_RENDER}.items():
        a = shaderbox_amd.sdf_ramp_scene(64, 36, 0.0)
        edit(a)
        assert shaderbox_amd.sdf_scene_check(a) is not None, case
        assert (shaderbox_amd.sdf_scene_check(a, program_only=True) is not None) == (case in BAD), case
        if 1 <= a.n_instr <= 32:
            assert M.check(M.from_block(bytes(a))) is not None, case
        b = shaderbox_amd.SdfSceneBuilder()
        b.s = a
        with pytest.raises(ValueError):
            b.scene()


def test_validator_accepts_programs_at_the_bounds():
    b = shaderbox_amd.SdfSceneBuilder(march_steps=512, checker_material=-1, shadow=1, view=1)
    for i in range(4):                                             # 4 x (4 primitives, 3 operators, OBJECT) = 32 instructions, depth 4
        for k in range(4):
            b.sphere((i, 1, k), .4, rot_axis=3)
        b.add().blend(.1).intersect().object(7 if i else 0)
    assert b.s.n_instr == 32 and b.check() is None and M.depth_of(M.from_block(bytes(b.scene()))) == 4
    with pytest.raises(ValueError):
        b.sphere((0, 0, 0), 1)                                     # a 33rd instruction
    assert shaderbox_amd.SdfSceneBuilder(march_steps=1, checker_material=7).plane((0, 1, 0), 0).object(0).check() is None


# ---- units: hand-stated values ----------------------------------------------------------------------------------------------------------

def value(I, p, extra=()):
    S = dict(M.ramp_scene(0.0), program=list(extra) + [I, M.obj(3)])
    d, m = M.sdf(S, *[np.array([c], dtype=F) for c in p])
    assert m[0] == 3
    return d[0]


def test_primitive_units():
    assert value(M.instr(M.PLANE, a=(0, 1, 0, .5)), (3, 2, 1)) == F(2.5)
    assert value(M.instr(M.SPHERE, (1, 0, 0), (1,)), (4, 4, 0)) == F(4)                       # |(3, 4, 0)| - 1
    assert value(M.instr(M.BOX, (0, 0, 0), (1, 2, 3)), (2, 0, 0)) == F(1) and value(M.instr(M.BOX, (0, 0, 0), (1, 2, 3)), (0, 0, 0)) == F(-1)
    assert value(M.instr(M.TORUS, (0, 0, 0), (2, .5)), (5, 0, 4)) == F(4.5)                   # |(5 - 2, 4)| - .5
    assert value(M.instr(M.Y_CYLINDER, (0, 0, 0), (1, 4)), (4, 0, 0)) == F(3) and value(M.instr(M.Y_CYLINDER, (0, 0, 0), (1, 4)), (0, 5, 0)) == F(3)
    # a cylinder from (0, 1, 0) to (0, 3, 0), radius .5, at distance 3 from its axis beside its middle: max(3, -(2 + 3), -(-2 - 1)) - .5
    assert value(M.instr(M.CYLINDER, (0, 0, 0), (0, 1, 0, .5), (0, 3, 0)), (3, 2, 0)) == F(2.5)
    assert value(M.instr(M.CAPSULE, (0, 0, 0), (0, 0, 0, .5), (0, 2, 0)), (3, 1, 0)) == F(2.5)
    assert value(M.instr(M.CAPSULE, (0, 0, 0), (0, 0, 0, .5), (0, 2, 0)), (0, 6, 0)) == F(3.5)
    # a Bezier in the plane z = 0, sampled off that plane above its end point a: .85 (|(0, 0, 2)| - .25)
    assert value(M.instr(M.BEZIER, (0, 0, 0), (-1, 0, 0, .25), (0, 1, 0), (1, 0, 0)), (-1, 0, 2)) == F(.85) * F(1.75)
    # offset, then rotation: the box's long x axis turned by rotate_around_z(90) — mul(q, M) takes q = (0, 2, 0) to (2, ~0, 0)
    d = value(M.instr(M.BOX, (5, 0, 0), (3, 1, 1), rot_axis=3, rot_deg=90.0), (5, 2, 0))
    assert d < 0 and value(M.instr(M.BOX, (5, 0, 0), (3, 1, 1)), (5, 2, 0)) == F(1)
    assert value(M.instr(M.BOX, (0, 0, 0), (1, 1, 3), rot_axis=1, rot_deg=-90.0), (0, 2, 0)) < 0     # x: y -> z
    assert value(M.instr(M.BOX, (0, 0, 0), (1, 1, 3), rot_axis=2, rot_deg=90.0), (2, 0, 0)) < 0      # y: x -> z


def test_operator_units():
    a, b = M.instr(M.PLANE, a=(0, 1, 0, 0)), M.instr(M.PLANE, a=(1, 0, 0, 0))                 # d1 = y, d2 = x
    p = (3, -2, 0)
    assert value(M.instr(M.ADD), p, (a, b)) == F(-2) and value(M.instr(M.INTERSECT), p, (a, b)) == F(3)
    assert value(M.instr(M.SUB), p, (a, b)) == F(-2) and value(M.instr(M.SUB), (-3, -2, 0), (a, b)) == F(3)      # max(d1, -d2)
    # op_blend(a, b, k): h = clamp(.5 + .5 (b - a) / k); at a == b, h = .5: a - k / 4
    assert value(M.instr(M.BLEND, a=(1,)), (2, 2, 0), (a, b)) == F(1.75)
    assert value(M.instr(M.BLEND, a=(1,)), p, (a, b)) == F(-2)                                # far apart: the minimum


def test_objects_fold_with_the_later_one_winning_ties_and_nans():
    P = [M.instr(M.PLANE, a=(0, 1, 0, 0)), M.obj(1), M.instr(M.PLANE, a=(0, 1, 0, 0)), M.obj(2), M.instr(M.PLANE, a=(0, 1, 0, 1)), M.obj(3)]
    S = dict(M.ramp_scene(0.0), program=P)
    d, m = M.sdf(S, *[np.array([0], dtype=F)] * 3)
    assert (d[0], m[0]) == (0, 2)                                  # 1 and 2 tie at 0: the later; 3 is farther
    S["program"] = P + [M.instr(M.PLANE, a=(float("nan"), 1, 0, 0)), M.obj(4)]
    d, m = M.sdf(S, *[np.array([0], dtype=F)] * 3)
    assert np.isnan(d[0]) and m[0] == 4
