"""GPU tests of SBX_APP_RAYTRACER_SCENE (include/sbx.h): k_raytracer_scene over the caller's scene, every comparison bit
for bit with NaN == NaN — against SBX_APP_RAYTRACER and its builds over the Cornell block, against the frames and points the
reference's own headers rendered with the fixture scenes written into them (tests/golden/raytracer_scenes/), and against
tests/raytracer_scene_model.py over random and edge scenes; then the layers above the kernel, the refusals and sbx_main_image's cache."""
import numpy as np
import pytest

import shaderbox_amd
from tests import raytracer_scene_model as M
from tests.app_checks import (assert_same, check_loopback_exchanges, check_rgba8, check_rows_host_rows_ranks_and_splits, edge_points,
                              frame_cache, run_sbx_render, same_tensor)
from tests.app_checks import renderer, variant_restored  # noqa: F401 (fixtures)
from tests.model_common import F

pytestmark = pytest.mark.gpu

APP = "raytracer_scene"
SIZES = [(64, 36), (67, 35)]

model_frame = frame_cache(lambda name, w, h: M.frame(M.scenes()[name], w, h))


def block(name):
    return M.to_block(M.scenes()[name])


# ---- the Cornell block through the scene kernel -----------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES)
def test_cornell_block_is_the_shipped_raytracer(renderer, size):
    w, h = size
    for t, mouse in [(0.0, (0.0, 0.0)), (0.5, (0.0, 0.0)), (3.1, (0.0, 0.0)), (0.5, (70.0, 3.0))]:
        before = renderer.raytracer_scene_launches()
        want = renderer.render("raytracer", w, h, t, mouse=mouse)
        assert renderer.raytracer_scene_launches() == before, "SBX_APP_RAYTRACER runs k_raytracer"
        same_tensor(renderer.render(APP, w, h, t, mouse=mouse), want, ("aux = None", t, mouse))
        a = shaderbox_amd.cornell_scene(w, h, t, mouse)
        same_tensor(renderer.render(APP, w, h, t, mouse=mouse, aux=a), want, ("the Cornell block", t, mouse))
        same_tensor(renderer.render(APP, w, h, -9.0, mouse=(3.0, 200.0), aux=a), want, "u_time and u_mouse are not read")
        assert renderer.raytracer_scene_launches() == before + 3, "the scene kernel ran, not k_raytracer"
        a.lighting = 1
        same_tensor(renderer.render(APP, w, h, t, aux=a), renderer.render("raytracer_phong", w, h, t, mouse=mouse), ("lighting = 1", t, mouse))
        a.lighting, a.shadow = 0, 0
        same_tensor(renderer.render(APP, w, h, t, aux=a), renderer.render("raytracer_noshadow", w, h, t, mouse=mouse), ("shadow = 0", t, mouse))
        rest = shaderbox_amd.cornell_scene(w, h, t, mouse, at_rest=True)
        same_tensor(renderer.render(APP, w, h, t, aux=rest), renderer.render("raytracer_static", w, h, t, mouse=mouse), ("at rest", t, mouse))


# ---- what the reference's headers rendered ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(M.scenes()))
def test_fixture_scenes_are_the_reference(renderer, variant_restored, name):
    import torch
    w, h = M.scene_table()["size"]
    fx, a = M.fixture(name), block(name)
    for variant in (0, 1):
        renderer.set_variant(variant)
        assert_same(renderer.render(APP, w, h, 0.0, aux=a), fx["frame"], (name, "frame", variant))
        assert_same(renderer.render_points(APP, w, h, 0.0, torch.from_numpy(fx["points"]), aux=a), fx["points_out"], (name, "points", variant))


# ---- random tame scenes against the model -------------------------------------------------------------------------------------------

FORCED = {0: (0, 0), 1: (16, 16), 2: (0, 16), 3: (16, 0)}
tame_frame = frame_cache(lambda seed, w, h: M.frame(M.tame_scene(seed, FORCED.get(seed)), w, h))


def test_tame_scenes_cover_what_they_should():
    scenes = [M.tame_scene(s, FORCED.get(s)) for s in range(20)]
    assert {(len(S["planes"]), len(S["spheres"])) for S in scenes} >= set(FORCED.values())
    assert {S["bounces"] for S in scenes} == set(range(1, 9))
    assert {(S["light_type"], S["lighting"]) for S in scenes} == {(1, 0), (2, 0), (1, 1), (2, 1)} and {S["shadow"] for S in scenes} == {0, 1}
    for S in scenes:
        assert all(np.isfinite(v).all() for v in (S["base"], S["rough"], S["ior"], S["refl"]))
        assert all(.1 <= r <= 2 and np.sqrt(sum((float(o[k]) - float(S["eye"][k])) ** 2 for k in range(3))) > r for o, r, _ in S["spheres"])


@pytest.mark.parametrize("seed", range(20))
def test_random_tame_scenes_are_the_model(renderer, seed):
    w, h = SIZES[seed % 2]
    S = M.tame_scene(seed, FORCED.get(seed))
    assert_same(renderer.render(APP, w, h, 0.0, aux=M.to_block(S)), tame_frame(seed, w, h), ("tame scene", seed, len(S["planes"]), len(S["spheres"])))


@pytest.mark.parametrize("seed", [1, 6, 15])
def test_default_witness_edge_and_ieee_kernels_agree(renderer, variant_restored, seed):
    w, h = SIZES[seed % 2]
    a = M.to_block(M.tame_scene(seed, FORCED.get(seed)))
    want = tame_frame(seed, w, h)
    for v in (0, 1, 2):
        renderer.set_variant(v)
        assert_same(renderer.render(APP, w, h, 0.0, aux=a), want, ("variant", v, seed))


# ---- numbers that are no scene --------------------------------------------------------------------------------------------------------

def edge_scene():
    """one block with: radius 0, a denormal radius, radius 1e30 and radius inf; a zero normal and a NaN normal component; distance inf;
    material ids -1, 8 and 2^31 - 1; ior -1 (Rn divides by 0); a plane through the eye (a hit at t = 0)"""
    S = dict(M.scenes()["tilted"])
    eye = S["eye"]
    floor, wall = S["planes"]
    # (after the NaN plane's hit, whose t is a NaN, `t > hit.t` is false for every later candidate: the wall replaces it for all rays)
    S["planes"] = [((F(0), F(0), F(0)), F(1), 3), ((F(0), F(1), F(0)), F("inf"), 2), ((F("nan"), F(0), F(-1)), F(-9), 1), wall, floor,
                   ((F(0), F(1), F(0)), eye[1], 7)]                       # dot(P0 - eye, n) = 0: every upward ray hits at t = 0, V = normalize(0)
    # (radius 1e30: its square is inf and so is dot(rc, rc), d2 is inf - inf; it lies BEHIND the eye, where `tca < 0` ends the test for the
    # primary rays, and is met by the shadow rays and reflections that head back)
    S["spheres"] = list(S["spheres"]) + [((F(1), F(1), F(2)), F(0), 3), ((F(-1), F(2), F(1)), F(1e-40), 3), ((F(0), F(0), F(2e30)), F(1e30), 1),
                                         ((F(3), F(1), F(0)), F("inf"), 2), ((F(-2.5), F(.5), F(1.5)), F(.5), -1), ((F(2.2), F(.5), F(2)), F(.5), 8),
                                         ((F(-2.2), F(2.5), F(0)), F(.6), 2 ** 31 - 1)]
    S["ior"] = S["ior"].copy()
    S["ior"][6] = F(-1)
    S["base"], S["rough"], S["refl"] = S["base"].copy(), S["rough"].copy(), S["refl"].copy()
    S["base"][7], S["rough"][7], S["ior"][7] = (.4, .4, .9), .3, 1.
    return S


edge_frame = frame_cache(lambda w, h: M.frame(edge_scene(), w, h))


def test_edge_scene_is_the_model(renderer, variant_restored):
    w, h = SIZES[1]
    S = edge_scene()
    a, want = M.to_block(S), edge_frame(w, h)
    assert (a.n_planes, a.n_spheres) == (6, 12)
    got = {}
    for v in (0, 1):
        renderer.set_variant(v)
        got[v] = renderer.render(APP, w, h, 0.0, aux=a).cpu().numpy()
        assert_same(got[v], want, ("edge scene, variant", v))
        assert M.nan_pixels(got[v]) == M.nan_pixels(want)
    assert M.nan_pixels(want) > 0 and (got[0][..., 3] == 1).all()


@pytest.mark.parametrize("radius,eye_x", [(1.5, 1e-40), (10.0, 5 * 2.0 ** -149), (1.5, 2.0 ** -126)])
def test_subnormal_sphere_normal_components(renderer, variant_restored, radius, eye_x):
    """(impact - origin) / radius with a quotient in the binary32 subnormal range, where the product with the radius's binary64
    reciprocal is not proved to be the IEEE quotient (5 * 2^-149 / 10 is an exact tie: IEEE 0, the product 2^-149): the fast pass records
    it and the wave re-runs.  The centre column of an odd-width frame, seen from an eye whose x is that small along -z, has rays with
    direction x = 0, so the hit's x is the eye's and dn.x = eye.x - 0."""
    w, h = SIZES[1]
    q = F(eye_x) / F(radius)
    assert F(eye_x) != 0 and abs(q) <= F(2.0 ** -126)
    S = dict(M.scenes()["tilted"], planes=[M.scenes()["tilted"]["planes"][0]], spheres=[((F(0), F(1), F(3) - F(radius)), F(radius), 3)],
             eye=(F(eye_x), F(1), F(6)), look_at=(F(eye_x), F(1), F(0)), fov=F(.5))
    m = {}
    want = M.frame(S, w, h, m)
    assert (m["first_kind"][:, w // 2] == 2).sum() >= 10, "the centre column meets the sphere"
    a = M.to_block(S)
    for v in (0, 1, 2):
        renderer.set_variant(v)
        assert_same(renderer.render(APP, w, h, 0.0, aux=a), want, ("subnormal normal component, variant", v, radius, eye_x))


def test_edge_points_are_the_model(renderer):
    import torch
    w, h = SIZES[0]
    pts = edge_points(w, h)
    S = M.scenes()["mirrors"]
    assert_same(renderer.render_points(APP, w, h, 0.0, torch.from_numpy(pts), aux=M.to_block(S)), M.points(S, w, h, pts), "edge points")


# ---- the layers above the kernel --------------------------------------------------------------------------------------------------------

def test_rows_host_rows_ranks_and_splits(renderer):
    w, h = SIZES[1]
    check_rows_host_rows_ranks_and_splits(renderer, APP, w, h, 0.0, model_frame("mirrors", w, h), cuts=[13, 14, 30], block_rows=8, aux=block("mirrors"))


def test_rgba8_frames(renderer):
    w, h = SIZES[1]
    assert_same(check_rgba8(renderer, APP, w, h, 0.0, aux=block("dirphong")), model_frame("dirphong", w, h), "the float frame")


def test_main_image_pixel_and_point(renderer):
    w, h = SIZES[0]
    a, S = block("noshadow"), M.scenes()["noshadow"]
    want = M.fixture("noshadow")["frame"]
    for x, y in [(0, 0), (40, 17), (63, 35)]:
        assert_same(np.array(renderer.main_image(APP, w, h, 0.0, (x + .5, y + .5), aux=a), dtype=F), want[y, x], ("pixel", x, y))
    pt = np.array([[40.25, 17.75]], dtype=F)
    assert_same(np.array(renderer.main_image(APP, w, h, 0.0, tuple(pt[0]), aux=a), dtype=F), M.points(S, w, h, pt)[0], "off-centre point")


def test_span_table_is_whole_rows():
    w, h = 256, 144
    for aux in (None, block("tilted")):
        table, pix, mw = shaderbox_amd.span_table(APP, w, h, 0.0, 8, 3, aux=aux)
        assert (table[:, 0] == 0).all() and (table[:, 1] == w).all() and mw == w and int(pix.sum()) == w * h


def test_exchanges_through_loopback_ranks(renderer):
    w, h = SIZES[0]
    check_loopback_exchanges(renderer, APP, 2, w, h, 0.37)


def test_sbx_render_host_reads_a_scene_file(tmp_path):
    w, h = SIZES[1]
    path = tmp_path / "scene.bin"
    path.write_bytes(bytes(block("tilted")))
    assert_same(run_sbx_render(tmp_path, APP, w, h, 0.0, flags=["--scene-bin", str(path)]), model_frame("tilted", w, h), "sbx_render --scene-bin")
    import os
    import subprocess
    (tmp_path / "short.bin").write_bytes(bytes(block("tilted"))[:-4])
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "host", "sbx_render")
    r = subprocess.run([exe, "--app", APP, "--res", "8x8", "--scene-bin", str(tmp_path / "short.bin")], capture_output=True, timeout=60)
    assert r.returncode == 2, "a file of another size is refused"


def test_captured_launch_replays(renderer):
    import torch
    w, h = SIZES[0]
    a = block("mirrors")
    out = torch.zeros((h, w, 4), dtype=torch.float32, device=renderer.tdev)
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            renderer.render(APP, w, h, 0.0, aux=a, out=out)
    a.bounces = 1                                                  # the block was read during the call: the graph holds its own copy
    out.fill_(-7.0)
    g.replay()
    torch.cuda.synchronize()
    assert_same(out, model_frame("mirrors", w, h), "graph replay")


# ---- refusals and the frame cache -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("field,value", [("n_planes", -1), ("n_planes", 17), ("n_spheres", -1), ("n_spheres", 17), ("bounces", 0), ("bounces", 9),
                                         ("light_type", 0), ("light_type", 3), ("lighting", -1), ("lighting", 2), ("shadow", -1), ("shadow", 2)])
def test_bad_blocks_are_refused_before_anything_is_enqueued(renderer, field, value):
    import torch
    w, h = SIZES[0]
    a = block("tilted")
    setattr(a, field, value)
    out = torch.full((h, w, 4), -7.0, dtype=torch.float32, device=renderer.tdev)
    launches = renderer.raytracer_scene_launches()
    with pytest.raises(shaderbox_amd.SbxError) as e:
        renderer.render(APP, w, h, 0.0, aux=a, out=out)
    assert e.value.code == shaderbox_amd.SBX_ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and renderer.raytracer_scene_launches() == launches


def test_main_image_cache_tells_scene_blocks_apart(renderer):
    """two blocks that differ only in their LAST sphere (byte 1344 of 1376) under the same uniforms: each call gets its own block's
    frame — the cache key holds the whole block (FrameCache::KEY_WORDS)"""
    w, h = SIZES[0]
    S = M.scenes()["tilted"]
    mk = lambda r: dict(S, spheres=list(S["spheres"]) + [((F(0), F(9), F(0)), F(.1), 1)] * 10 + [((F(0), F(1.6), F(2.5)), F(r), 3)])  # noqa: E731
    Sa, Sb = mk(.5), mk(.9)
    a, b = M.to_block(Sa), M.to_block(Sb)
    assert a.n_spheres == 16 and bytes(a)[:1344] == bytes(b)[:1344] and bytes(a) != bytes(b)
    fa, fb = M.frame(Sa, w, h), M.frame(Sb, w, h)
    ys, xs = np.nonzero((~M.same_bits(fa, fb)).any(axis=-1))
    assert len(xs) > 10
    x, y = int(xs[len(xs) // 2]), int(ys[len(xs) // 2])
    renderer.reset_stats()
    for blk, want in ((a, fa), (b, fb), (a, fa), (b, fb)):
        assert_same(np.array(renderer.main_image(APP, w, h, 0.0, (x + .5, y + .5), aux=blk), dtype=F), want[y, x], "its own block's pixel")
    st = renderer.stats()
    assert st["main_image_frames"] == 2 and st["main_image_hits"] == 2
