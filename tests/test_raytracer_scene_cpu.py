"""CPU tests of SBX_APP_RAYTRACER_SCENE's definition (tests/raytracer_scene_model.py; include/sbx.h): over the Cornell
block it is the oracle's `raytracer` in every bit, over the scenes of tests/golden/raytracer_scenes.json it is what the reference's
own headers rendered with those scenes written into them (tools/make_golden_raytracer_scenes.py), and the block's Python layout is
the C header's."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import shaderbox_amd
from tests import raytracer_builds_model as B
from tests import raytracer_scene_model as M
from tests.model_common import F, oracle, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def differing(a, b):
    return int((~same_bits(a, b)).any(axis=-1).sum())


@pytest.mark.parametrize("size", [(64, 36), (61, 35)])
@pytest.mark.parametrize("t,mouse", [(0.0, (0.0, 0.0)), (0.5, (0.0, 0.0)), (3.1, (0.0, 0.0)), (0.5, (70.0, 3.0))])
def test_model_over_the_cornell_block_is_the_oracle(size, t, mouse):
    from oracle.oracle import APP_IDS
    w, h = size
    S = M.from_block(shaderbox_amd.cornell_scene(w, h, t, mouse))
    assert (len(S["planes"]), len(S["spheres"]), S["bounces"], S["light_type"], S["lighting"], S["shadow"]) == (6, 3, 2, 1, 0, 1)
    assert differing(M.frame(S, w, h), oracle().render(APP_IDS["raytracer"], w, h, t, mouse=mouse)) == 0


def test_cornell_block_at_rest_is_the_static_build():
    """at_rest against what the reference's header rendered with its `#if 1` at :29 off (tests/golden/raytracer_builds/)"""
    for w, h, t, mouse, want in B.fixture("static")["frames"]:
        a = shaderbox_amd.cornell_scene(w, h, t, mouse, at_rest=True)
        assert bytes(a) == bytes(shaderbox_amd.cornell_scene(w, h, t + 1.25, mouse, at_rest=True)), "at rest, u_time is not read"
        assert differing(M.frame(M.from_block(a), w, h), want) == 0, (w, h, t, mouse)
    moving, still = shaderbox_amd.cornell_scene(64, 36, 0.5), shaderbox_amd.cornell_scene(64, 36, 0.5, at_rest=True)
    assert list(still.spheres[1].origin) == [0.75, 1.0, -0.75] and list(still.light_L)[2] == 0.0 and list(moving.light_L)[2] == 1.5
    assert bytes(moving) != bytes(still)


def test_cornell_block_switches_are_the_other_builds():
    """lighting = 1 and shadow = 0 on the Cornell block against the frames of the Phong and unshadowed builds of the reference's header"""
    for build, change in (("phong", dict(lighting=1)), ("noshadow", dict(shadow=0))):
        w, h, t, mouse, want = B.fixture(build)["frames"][0]
        S = dict(M.from_block(shaderbox_amd.cornell_scene(w, h, t, mouse)), **change)
        assert differing(M.frame(S, w, h), want) == 0, build


@pytest.fixture(scope="module")
def fixture_frames():
    table = M.scene_table()
    w, h = table["size"]
    frames, masks = {}, {}
    for name, S in M.scenes().items():
        masks[name] = {}
        frames[name] = M.frame(S, w, h, masks[name])
    return table, frames, masks


def test_model_is_the_reference_over_the_fixture_scenes(fixture_frames):
    table, frames, _ = fixture_frames
    w, h = table["size"]
    for e in table["scenes"]:
        name, S, fx = e["name"], M.scene_of(e), M.fixture(e["name"])
        assert set(fx.files) == {"frame", "points", "points_out"}
        assert fx["frame"].shape == (h, w, 4) and (fx["frame"][..., 3] == 1).all()
        assert differing(frames[name], fx["frame"]) == 0, name
        assert np.array_equal(fx["points"], M.fixture_points(e["points_seed"], w, h, table["points"]))
        assert not (fx["points"] - np.floor(fx["points"]) == .5).all(axis=1).any(), "off-centre points"
        assert differing(M.points(S, w, h, fx["points"]), fx["points_out"]) == 0, (name, "points")


def test_fixtures_say_something(fixture_frames):
    """the conditions of the committed files: asserted from the model's masks, as the tool asserted them when it recorded"""
    table, frames, masks = fixture_frames
    M.check_conditions(table, {n: M.fixture(n)["frame"] for n in frames}, masks)
    by = {e["name"]: e for e in table["scenes"]}
    def facing_mirrors(e):                          # two planes of opposite normals whose materials reflect
        S = M.scene_of(e)
        mirrors = [n for n, _, mat in S["planes"] if 0 <= mat < 8 and S["refl"][mat] > 0]
        return any(tuple(-c for c in a) == tuple(b) for a in mirrors for b in mirrors)
    assert any(e["bounces"] == 4 and facing_mirrors(e) for e in by.values())
    shipped = shaderbox_amd.cornell_scene(64, 36, 0.0)
    for e in by.values():                           # a camera and a FOV other than the shipped ones
        S = M.scene_of(e)
        assert tuple(S["eye"]) != tuple(F(v) for v in shipped.eye) and S["fov"] != F(shipped.fov)
    tilted = [p for e in by.values() for p in e["planes"] if sum(float.fromhex(c) != 0 for c in p["direction"]) == 3]
    assert tilted and abs(sum(float.fromhex(c) ** 2 for c in tilted[0]["direction"]) - 1) > .05, "a non-axis, non-unit plane normal"
    largest = max(os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden")) if f.endswith(".npz"))
    w, h = table["size"]
    for n in by:
        assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "raytracer_scenes", "%s_%dx%d.npz" % (n, w, h))) <= largest


def test_table_holds_settings_only():
    def leaves(x):
        if isinstance(x, dict):
            for v in x.values():
                yield from leaves(v)
        elif isinstance(x, list):
            for v in x:
                yield from leaves(v)
        else:
            yield x
    table = M.scene_table()
    for e in table["scenes"]:
        for key, v in e.items():
            for leaf in leaves(v):
                if key in ("name",):
                    assert leaf.isidentifier()
                elif isinstance(leaf, str):
                    assert np.isfinite(float.fromhex(leaf)) and F(float.fromhex(leaf)) == float.fromhex(leaf), (e["name"], key, leaf)
                else:
                    assert isinstance(leaf, int)


LAYOUT = r'''
#include "sbx.h"
#include <cstdio>
#define O(f) (int)offsetof(sbx_aux_raytracer_scene, f)
int main() { printf("%d %d %d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d  %d %d %d  %d %d %d\n",
    (int)sizeof(sbx_aux_raytracer_scene), (int)sizeof(sbx_rt_material), (int)sizeof(sbx_rt_plane), (int)sizeof(sbx_rt_sphere),
    O(eye), O(fov), O(look_at), O(bounces), O(light_L), O(light_type), O(light_color), O(lighting), O(ambient), O(shadow), O(n_planes), O(n_spheres),
    O(materials), O(planes), O(spheres),
    (int)offsetof(sbx_rt_material, metallic), (int)offsetof(sbx_rt_material, roughness), (int)offsetof(sbx_rt_material, ior),
    (int)offsetof(sbx_rt_material, reflectivity), (int)offsetof(sbx_rt_material, translucency),
    (int)offsetof(sbx_rt_plane, direction), (int)offsetof(sbx_rt_plane, distance), (int)offsetof(sbx_rt_plane, material),
    (int)offsetof(sbx_rt_sphere, origin), (int)offsetof(sbx_rt_sphere, radius), (int)offsetof(sbx_rt_sphere, material)); return SBX_APP_RAYTRACER_SCENE == 32 && SBX_ABI_VERSION == 2 ? 0 : 1; }
'''


def test_ctypes_layout_is_the_headers(tmp_path):
    src, exe = tmp_path / "layout.cpp", str(tmp_path / "layout")
    src.write_text(LAYOUT)
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src)], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    A, Mt, P, Sp = shaderbox_amd.RaytracerScene, shaderbox_amd.RtMaterial, shaderbox_amd.RtPlane, shaderbox_amd.RtSphere
    want = [ctypes.sizeof(A), ctypes.sizeof(Mt), ctypes.sizeof(P), ctypes.sizeof(Sp)]
    want += [getattr(A, f).offset for f in ("eye", "fov", "look_at", "bounces", "light_L", "light_type", "light_color", "lighting", "ambient", "shadow",
                                            "n_planes", "n_spheres", "materials", "planes", "spheres")]
    want += [getattr(Mt, f).offset for f in ("metallic", "roughness", "ior", "reflectivity", "translucency")]
    want += [getattr(P, f).offset for f in ("direction", "distance", "material")] + [getattr(Sp, f).offset for f in ("origin", "radius", "material")]
    assert got == want and got[:4] == [1376, 32, 32, 32]
    assert shaderbox_amd.app_id("raytracer_scene") == shaderbox_amd.APP_RAYTRACER_SCENE == 32 == shaderbox_amd.ALL_APPS["APP_RAYTRACER_SCENE"]
    assert shaderbox_amd.RT_MAX_PLANES == shaderbox_amd.RT_MAX_SPHERES == 16


def test_blocks_round_trip_and_the_builder_fills_counts():
    for S in M.scenes().values():
        a = M.to_block(S)
        assert (a.n_planes, a.n_spheres) == (len(S["planes"]), len(S["spheres"]))
        assert bytes(M.to_block(M.from_block(a))) == bytes(a)
    a = shaderbox_amd.raytracer_scene(planes=[((0, -1, 0), 0.0, 1)], spheres=[((0, 1, 0), 1.0, 2), ((2, 1, 0), 0.5, 0)],
                                      materials={1: dict(base_color=(.5, .5, .5)), 2: dict(base_color=(1, 0, 0), reflectivity=1.0, roughness=.1)},
                                      light=(0, 4, 2), eye=(0, 1, 5), look_at=(0, 1, 0), fov=0.5, bounces=3, lighting=shaderbox_amd.LIGHTING_PHONG)
    assert (a.n_planes, a.n_spheres, a.bounces, a.lighting, a.shadow, a.light_type) == (1, 2, 3, 1, 1, shaderbox_amd.LIGHT_POINT)
    assert a.materials[1].ior == 1.0 and a.materials[2].roughness == F(.1) and list(a.ambient) == [F(.01)] * 3 and a.spheres[1].material == 0
    with pytest.raises(ValueError):
        shaderbox_amd.raytracer_scene(planes=[((0, 1, 0), 0.0, 1)] * 17)


def test_model_units():
    S = M.scenes()["mirrors"]
    w, h = 32, 18
    empty = M.frame(dict(S, planes=[], spheres=[]), w, h)
    assert (empty[..., :3] == 0).all() and (empty[..., 3] == 1).all(), "no primitive: the background, black"
    m = {}
    M.frame(dict(S, bounces=1), w, h, m)
    assert int(m["depth"].max()) == 1, "bounces = 1 never reflects"
    m4 = {}
    M.frame(S, w, h, m4)
    assert int(m4["depth"].max()) == 4 and (m4["first_kind"] == m["first_kind"]).all()
    # a material-0 sphere is drawn flat and casts no shadow; a material -1 sphere (mat_invalid) is never intersected
    bulb = dict(S, spheres=[((F(0), F(1), F(0)), F(1), 0)], shadow=1)
    mb, mn = {}, {}
    fb = M.frame(bulb, w, h, mb)
    assert int(mb["shadowed"].sum()) == 0 and int((mb["first_mat"] == 0).sum()) > 0
    flat = M.frame(dict(bulb, shadow=0), w, h)      # (the walls may still shadow a bulb's pixel: the shadow ray is for another check)
    moved = M.frame(dict(bulb, shadow=0, light=(F(-1), F(1), F(2)), lighting=1, ambient=(F(.5), F(.5), F(.5))), w, h)
    on = mb["first_mat"] == 0                       # (1 - f) * materials[0].base_color: no light, no lighting model, no ambient enters
    assert same_bits(flat[on], moved[on]).all() and not same_bits(flat[~on], moved[~on]).all()
    M.frame(dict(S, spheres=[((F(0), F(1), F(0)), F(1), -1)]), w, h, mn)
    assert int((mn["first_kind"] == 2).sum()) == 0
