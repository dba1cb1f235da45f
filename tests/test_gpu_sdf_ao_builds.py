"""GPU tests of SBX_APP_SDF_AO_SHADOW and SBX_APP_SDF_AO_NORMALS (src/app_sdf_ao.h with one of its `#if 0` blocks on; include/sbx.h,
DESIGN.md §5.11): every layer bit for bit, NaN == NaN, all four channels, against tests/sdf_ao_builds_model.py — and, at 64x36,
against the frames the edited reference header rendered (tests/golden/sdf_ao_builds/)."""
import os
import subprocess

import numpy as np
import pytest

from tests import sdf_ao_builds_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["shadow", "normals"]
F = np.float32


@pytest.fixture(scope="module")
def renderer():
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


_FRAMES = {}


def model_frame(build, w, h, t, aux=None):
    key = (build, w, h, t, aux)
    if key not in _FRAMES:
        _FRAMES[key] = M.frame(build, w, h, t, aux)
    return _FRAMES[key]


def aux_block(aux):
    import shaderbox_amd
    if aux is None:
        return None
    a = shaderbox_amd.AuxSdfAo()
    a.fog_density, a.fog_falloff = aux
    return a


def assert_same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = M.same_bits(got, want)
    if not ok.all():
        i = np.argwhere(~ok)[:3]
        raise AssertionError("%s: %d differing channels, first %s: got %s want %s"
                             % (what, int((~ok).sum()), i.tolist(), [got[tuple(j)] for j in i], [want[tuple(j)] for j in i]))


def golden(build):
    z = np.load(os.path.join(ROOT, "tests", "golden", "sdf_ao_builds", "sdf_ao_%s_64x36.npz" % build))
    return [(float(u[4]), z["t%g" % u[4]]) for u in z["uniforms"]]


# u_mouse does not enter app_sdf_ao.h: every mouse value gives the frame of (0, 0).  Fog falloff 0 makes the factor 0 / 0: a NaN frame.
CASES = [(0.37, (0.0, 0.0), None), (2.5, (300.0, 120.0), None), (4.6, (-3.0, 1e6), (0.3, 0.0)), (9.25, (0.0, 0.0), (0.02, 1.5)),
         (-3.1, (7.0, 7.0), (-0.2, 0.25))]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (64, 36), (257, 130), (640, 360)])
def test_frames(renderer, build, w, h):
    for t, mouse, aux in CASES:
        want = model_frame(build, w, h, t, aux)
        assert (want[..., 3] == 1).all()
        if aux is not None and aux[1] == 0.0:
            assert np.isnan(want[..., :3]).all()
        assert_same(renderer.render("sdf_ao_" + build, w, h, t, mouse=mouse, aux=aux_block(aux)), want, (build, w, h, t, mouse, aux))


@pytest.mark.parametrize("build", BUILDS)
def test_frames_1080p(renderer, build):
    w, h = 1920, 1080
    for t, aux in [(1.3, None), (5.9, (0.05, 0.8))][:1 if build == "normals" else 2]:
        assert_same(renderer.render("sdf_ao_" + build, w, h, t, aux=aux_block(aux)), model_frame(build, w, h, t, aux), (build, w, h, t, aux))


@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames(renderer, build):
    """the frames src/app_sdf_ao.h itself rendered with the one `#if 0` turned on, in every kernel form"""
    try:
        for variant in (0, 1, 2, 3):
            renderer.set_variant(variant)
            for t, want in golden(build):
                assert_same(renderer.render("sdf_ao_" + build, 64, 36, t), want, (build, t, "variant", variant))
    finally:
        renderer.set_variant(0)


def test_shipped_build_still_equals_the_oracle(renderer, oracle):
    from oracle.oracle import APP_SDF_AO
    w, h, t = 320, 180, 2.5
    want = oracle.render(APP_SDF_AO, w, h, t)
    assert_same(renderer.render("sdf_ao", w, h, t), want, "sdf_ao")
    assert_same(model_frame("default", w, h, t), want, "model")
    for build in BUILDS:                                                 # and the new apps are other frames
        assert not M.same_bits(renderer.render("sdf_ao_" + build, w, h, t).cpu().numpy(), want).all()


def _points(w, h):
    rng = np.random.default_rng(11)
    big = float(2 ** 24) * w
    return np.concatenate([
        rng.uniform(0, 1, size=(400, 2)) * [w, h],                      # off-centre
        rng.uniform(-3, 4, size=(300, 2)) * [w, h],                     # negative and outside the frame
        rng.uniform(-1, 1, size=(50, 2)) * [big, big * 16],
        [[0, 0], [w, h], [-.5, -.5], [w - .5, h - .5], [-1, 7], [big, 3], [3, -big], [1e30, 1e30], [-3e38, 5], [3e38, -3e38]],
        [[np.inf, 5], [5, -np.inf], [np.inf, np.inf], [np.nan, 5], [5, np.nan], [np.nan, np.nan], [np.inf, np.nan]],
    ]).astype(np.float32)


@pytest.mark.parametrize("build", BUILDS)
def test_points_and_main_image(renderer, build):
    import torch
    app = "sdf_ao_" + build
    w, h = 1920, 1080
    pts = _points(w, h)
    for t, aux in [(2.5, None), (0.37, (0.3, 0.7))]:
        a = aux_block(aux)
        want = M.main_image(build, w, h, t, pts[:, 0], pts[:, 1], aux)
        assert_same(renderer.render_points(app, w, h, t, torch.from_numpy(pts), aux=a), want, (build, "points", t))
        assert_same(renderer.main_image_batch(app, w, h, t, pts[:64], aux=a), want[:64], (build, "batch", t))
        for i in [0, 1, 400, 701, 750, 755, len(pts) - 1, len(pts) - 4]:
            c = renderer.main_image(app, w, h, t, (float(pts[i, 0]), float(pts[i, 1])), aux=a)
            assert_same(np.asarray(c, dtype=np.float32), want[i], (build, "main_image", i))
    w, h, t = 640, 360, 2.5                                              # pixel centres: served from the cached frame, per aux block
    for aux in (None, (0.3, 0.0), (0.02, 1.5)):
        c = renderer.main_image(app, w, h, t, (10.5, 20.5), aux=aux_block(aux))
        assert_same(np.asarray(c, dtype=np.float32), M.main_image(build, w, h, t, F(10.5), F(20.5), aux), (build, "centre", aux))


@pytest.mark.parametrize("build", BUILDS)
def test_variants_same_bits(renderer, build):
    import torch
    app = "sdf_ao_" + build
    w, h, t = 1920, 1080, 1.3
    pts = torch.from_numpy(_points(w, h))
    got = {}
    try:
        for v in (0, 1, 2, 3):
            renderer.set_variant(v)
            got[v] = (renderer.render(app, w, h, t).cpu().numpy(), renderer.render_points(app, w, h, t, pts).cpu().numpy())
    finally:
        renderer.set_variant(0)
    for v in (1, 2, 3):
        assert_same(got[v][0], got[0][0], (build, "frame variant 0 vs", v))
        assert_same(got[v][1], got[0][1], (build, "points variant 0 vs", v))
    assert_same(got[0][0], model_frame(build, w, h, t), (build, "frame vs model"))


@pytest.mark.parametrize("build", BUILDS)
def test_extreme_times_run_the_plain_kernel(renderer, build):
    """beyond |u_time| = 1e8, and for inf / NaN, the camera's rotation is whatever the spec's reduction returns and the plain kernel
    runs (sbx_capi.hip tame_time): same operations as the model on whatever the matrix is"""
    for t in (3e8, -1e30, float("inf"), float("nan")):
        assert_same(renderer.render("sdf_ao_" + build, 64, 36, t), M.frame(build, 64, 36, t), (build, t))


@pytest.mark.parametrize("build", BUILDS)
def test_rows_host_rows_ranks_and_splits(renderer, build):
    import torch
    from shaderbox_amd import shard
    app = "sdf_ao_" + build
    w, h, br, t = 640, 360, 8, 2.5
    aux = (0.02, 1.5)
    a = aux_block(aux)
    whole = renderer.render(app, w, h, t, aux=a)
    assert_same(whole, model_frame(build, w, h, t, aux), "whole")
    parts = [renderer.render(app, w, h, t, aux=a, rows=(r0, r1)) for r0, r1 in [(0, 13), (13, 14), (14, 300), (300, h)]]
    assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32)), "rows"
    host = np.zeros((h, w, 4), dtype=np.float32)
    renderer.render_to_host(app, w, h, t, host, aux=a)
    assert np.array_equal(host.view(np.uint32), whole.cpu().numpy().view(np.uint32)), "host rows"
    for n in (2, 3):
        for rr, rounds in [(1, 1), (1, 2)]:
            rows_max = shard.rank_rows_max(h, br, n, rr, rounds)
            gathered = torch.empty((n * rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
            for r in range(n):
                renderer.render_rank(app, w, h, t, br, r, n, aux=a, out=gathered[r * rows_max:(r + 1) * rows_max], root_rounds=rr, rounds=rounds)
            frame = renderer.assemble(gathered, w, h, br, n, root_rounds=rr, rounds=rounds)
            assert torch.equal(frame.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, "rank + assemble")
            for ch in (4, 3):
                inplace = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                if ch == 3:
                    inplace[..., 3] = 1.0
                for r in range(n):
                    renderer.render_rank_in_place(app, w, h, t, br, r, n, inplace, aux=a, root_rounds=rr, rounds=rounds, channels=ch)
                assert torch.equal(inplace.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, ch, "in place")
            for ch in (4, 3):                                            # slab pieces, four channels and sbx_render_split_rgb
                slabs = torch.empty((n, rows_max, w, ch), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 0, 5, slabs[r], aux=a, root_rounds=rr, rounds=rounds)
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 5, rows_max, slabs[r], aux=a, root_rounds=rr, rounds=rounds)
                root = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                renderer.render_rank_in_place(app, w, h, t, br, 0, n, root, aux=a, root_rounds=rr, rounds=rounds)
                renderer.assemble_peers(slabs[1:].contiguous(), w, h, br, n, root, root_rounds=rr, rounds=rounds)
                assert torch.equal(root.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, ch, "peers")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, build, n):
    """the span exchange (whole rows: no cost model, as APP_SDF_AO) and the direct exchange's rgb slabs, every rank's schedule on this GPU"""
    import torch
    from shaderbox_amd.distributed import LoopbackWorld
    app = "sdf_ao_" + build
    w, h, t = 1000, 333, 2.5
    full = renderer.render(app, w, h, t)
    for exchange, groups, relief in [("spans", 1, (1, 1)), ("spans", 2, (1, 2)), ("direct", 1, (1, 1))]:
        world = LoopbackWorld(n)
        plans = world.plans(renderer, w, h, block_rows=8, groups=groups, root_rounds=relief[0], rounds=relief[1], exchange=exchange)
        plans[0].frame.fill_(-7.0)
        got = LoopbackWorld.render(plans, app, t)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), full.view(torch.int32)), (n, exchange, groups, relief)


@pytest.mark.parametrize("build", BUILDS)
def test_rgba8_frames(renderer, build):
    app = "sdf_ao_" + build
    w, h, t = 800, 450, 2.5
    try:
        renderer.set_output_format("rgba32f")
        f = renderer.render(app, w, h, t)
        packed = renderer.pack_unorm8(f, flip_y=False)
        renderer.set_output_format("rgba8")
        got = renderer.render(app, w, h, t)
        assert np.array_equal(got.cpu().numpy(), packed.cpu().numpy())
        assert (got.cpu().numpy()[..., 3] == 255).all()
    finally:
        renderer.set_output_format("rgba32f")


def test_precision_tier_is_ignored(renderer):
    w, h, t = 257, 130, 2.5
    try:
        for build in BUILDS:
            renderer.set_precision("exact")
            a = renderer.render("sdf_ao_" + build, w, h, t).cpu().numpy()
            renderer.set_precision("1e-4")
            assert_same(renderer.render("sdf_ao_" + build, w, h, t), a, (build, "tier"))
    finally:
        renderer.set_precision("exact")


@pytest.mark.parametrize("build", BUILDS)
def test_multi_render(renderer, build):
    import torch
    import shaderbox_amd
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("sbx_multi_render across devices needs 2 or more visible GPUs (%d visible)" % ndev)
    w, h, t = 1280, 720, 2.5
    m = shaderbox_amd.MultiRenderer(list(range(ndev)))
    try:
        got = m.render("sdf_ao_" + build, w, h, t)
        torch.cuda.synchronize()
        assert_same(got, model_frame(build, w, h, t), "multi")
    finally:
        m.close()


DROPIN = r'''
#include "sbx_mainimage.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>
struct vec2 { float x, y; float operator[](int i) const { return i ? y : x; } };
struct vec4 { float v[4]; float& operator[](int i) { return v[i]; } };
int main(int argc, char** argv) {
    const int W = atoi(argv[1]), H = atoi(argv[2]);
    iResolution[0] = (float)W; iResolution[1] = (float)H;
    iGlobalTime = (float)atof(argv[3]);
    std::vector<float> px((size_t)W * H * 4);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            vec4 c;
            mainImage(c, vec2{x + .5f, y + .5f});
            for (int k = 0; k < 4; ++k) px[((size_t)y * W + x) * 4 + k] = c[k];
        }
    FILE* f = fopen(argv[4], "wb");
    fwrite(px.data(), sizeof(float), px.size(), f);
    fclose(f);
    return 0;
}
'''


@pytest.mark.parametrize("build", BUILDS)
def test_cpp_dropin(tmp_path, build):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = tmp_path / "dropin.cpp"
    src.write_text(DROPIN)
    lib = os.path.join(ROOT, "shaderbox_amd", "lib")
    exe = str(tmp_path / ("APP_SDF_AO_" + build.upper()))
    # -DAPP_SDF_AO beside it, as a project that only adds the build's define would have: the build's define is tested first
    subprocess.run(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-DAPP_SDF_AO", "-DAPP_SDF_AO_" + build.upper(),
                    "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(rocm, "include"), "-o", exe, str(src), "-L" + lib, "-lsbx", "-L" + os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    for w, h, t in [(320, 180, 0.37), (97, 61, 9.25)]:
        out = str(tmp_path / "px.f32")
        subprocess.run([exe, str(w), str(h), repr(t), out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
        assert_same(got, model_frame(build, w, h, t), ("dropin", build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    exe = os.path.join(ROOT, "host", "sbx_render")
    assert os.path.exists(exe), "host/sbx_render is built by build()"
    w, h = 257, 130
    for t, aux, flags in [(0.37, None, []), (2.5, (0.25, 1.5), ["--fog-density", "0.25", "--fog-falloff", "1.5"])]:
        out = str(tmp_path / "frame.f32")
        subprocess.run([exe, "--app", "sdf_ao_" + build, "--res", "%dx%d" % (w, h), "--time", repr(t), "--f32", out] + flags, check=True, timeout=120)
        raw = np.fromfile(out, dtype=np.float32)
        assert raw.size == w * h * 4
        assert_same(raw.reshape(h, w, 4), model_frame(build, w, h, t, aux), ("sbx_render --app sdf_ao_" + build, t, aux))
