"""GPU tests of SBX_APP_EGG_STRAIGHT and SBX_APP_EGG_OVAL (src/app_egg.h without its `#define BEZIER` / with its `#if 1` at :46 off;
include/sbx.h): every layer bit for bit, NaN == NaN, all four channels, against tests/egg_builds_model.py — and
against the frames and points the edited reference header rendered (tests/golden/egg_builds/)."""
import os
import subprocess

import numpy as np
import pytest

from tests import egg_builds_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["straight", "oval"]
F = np.float32
TIMES = (0.0037, 0.2, -0.41, 1.3)                                       # at 1.3 the turntable has carried the figure out of view


@pytest.fixture(scope="module")
def renderer():
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


_FRAMES = {}


def model_frame(build, w, h, t):
    key = (build, w, h, t)
    if key not in _FRAMES:
        _FRAMES[key] = M.frame(build, w, h, t, threads=16)
    return _FRAMES[key]


def assert_same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = M.same_bits(got, want)
    if not ok.all():
        i = np.argwhere(~ok)[:3]
        raise AssertionError("%s: %d differing channels, first %s: got %s want %s"
                             % (what, int((~ok).sum()), i.tolist(), [got[tuple(j)] for j in i], [want[tuple(j)] for j in i]))


def golden(build):
    z = np.load(os.path.join(ROOT, "tests", "golden", "egg_builds", "egg_%s.npz" % build))
    return [(float(u[4]), z["t%g" % u[4]]) for u in z["uniforms"]], z["points"], z["points_uniforms"], z["points_out"]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (96, 54), (257, 130), (640, 360)])
def test_frames(renderer, build, w, h):
    for t in TIMES:
        want = model_frame(build, w, h, t)
        assert (want[..., 3] == 1).all()
        assert_same(renderer.render("egg_" + build, w, h, t, mouse=(300.0, 120.0)), want, (build, w, h, t))   # u_mouse does not enter


@pytest.mark.parametrize("build", BUILDS)
def test_frames_1080p(renderer, build):
    w, h, t = 1920, 1080, 0.02
    assert_same(renderer.render("egg_" + build, w, h, t), model_frame(build, w, h, t), (build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames_and_points(renderer, build):
    """what src/app_egg.h itself rendered with the one line edited, in every kernel form"""
    import torch
    frames, pts, u, want = golden(build)
    try:
        for variant in (0, 1, 2, 3):
            renderer.set_variant(variant)
            for t, g in frames:
                assert_same(renderer.render("egg_" + build, 96, 54, t), g, (build, t, "variant", variant))
            got = renderer.render_points("egg_" + build, int(u[0]), int(u[1]), float(u[4]), torch.from_numpy(pts))
            assert_same(got, want, (build, "points", "variant", variant))
    finally:
        renderer.set_variant(0)


def test_shipped_build_still_equals_the_oracle(renderer, oracle):
    from oracle.oracle import APP_EGG
    w, h, t = 320, 180, 0.2
    want = oracle.render(APP_EGG, w, h, t)
    assert_same(renderer.render("egg", w, h, t), want, "egg")
    assert_same(model_frame("default", w, h, t), want, "model")
    others = []
    for build in BUILDS:                                                 # and the new apps are other frames
        others.append(renderer.render("egg_" + build, w, h, t).cpu().numpy())
        assert not M.same_bits(others[-1], want).all()
    assert not M.same_bits(others[0], others[1]).all()


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
def test_variants_same_bits(renderer, build):
    import torch
    app = "egg_" + build
    w, h, t = 1920, 1080, 0.02
    pts = _points(w, h)
    got = {}
    try:
        for v in (0, 1, 2, 3):
            renderer.set_variant(v)
            got[v] = (renderer.render(app, w, h, t).cpu().numpy(), renderer.render_points(app, w, h, t, torch.from_numpy(pts)).cpu().numpy())
    finally:
        renderer.set_variant(0)
    for v in (1, 2, 3):
        assert_same(got[v][0], got[0][0], (build, "frame variant 0 vs", v))
        assert_same(got[v][1], got[0][1], (build, "points variant 0 vs", v))
    assert_same(got[0][0], model_frame(build, w, h, t), (build, "frame vs model"))
    assert_same(got[0][1], M.main_image(build, w, h, t, pts[:, 0], pts[:, 1]), (build, "points vs model"))
    assert_same(renderer.main_image_batch(app, w, h, t, pts[:64]), got[0][1][:64], (build, "batch"))
    for i in [0, 1, 400, 701, 750, 755, len(pts) - 1, len(pts) - 4]:
        c = renderer.main_image(app, w, h, t, (float(pts[i, 0]), float(pts[i, 1])))
        assert_same(np.asarray(c, dtype=np.float32), got[0][1][i], (build, "main_image", i))


def test_main_image_centre_hits_alternate_between_the_builds(renderer):
    """sbx_main_image serves a pixel centre from the frame cached for (app, uniforms): the three builds, asked in turn on one context
    with equal uniforms, each get their own pixel — at pixels where the builds' frames differ"""
    w, h, t = 96, 54, 0.02
    frames = {b: model_frame(b, w, h, t) for b in M.BUILDS}
    pixels = []
    for b in BUILDS:
        ys, xs = np.nonzero(~M.same_bits(frames[b], frames["default"]).all(axis=2))
        assert len(xs) > 0
        pixels += [(int(xs[0]), int(ys[0])), (int(xs[-1]), int(ys[-1]))]
    for _ in range(2):
        for x, y in pixels:
            for b in M.BUILDS:
                c = renderer.main_image(M.APP_OF[b], w, h, t, (x + .5, y + .5))
                assert_same(np.asarray(c, dtype=np.float32), frames[b][y, x], (b, "centre", x, y))


def test_full_frames_alternate_between_the_builds(renderer):
    """a dispatch-order table is keyed by the app: back-to-back launches of one standing scene, the builds taking turns in runs long
    enough for a table to be built and adopted, keep returning each build's own frame"""
    w, h, t = 1920, 1080, 0.02
    first = {}
    for rnd in range(2):
        for b in M.BUILDS:
            for k in range(6):
                got = renderer.render(M.APP_OF[b], w, h, t)
                if b not in first:
                    first[b] = got.clone()
            assert_same(got, first[b].cpu().numpy(), (b, "round", rnd))
    for b in BUILDS:
        assert_same(first[b], model_frame(b, w, h, t), (b, "vs model"))
        assert not M.same_bits(first[b].cpu().numpy(), first["default"].cpu().numpy()).all()


@pytest.mark.parametrize("build", BUILDS)
def test_extreme_times_run_the_plain_kernel(renderer, build):
    """beyond |u_time| = 1e8, and for inf / NaN, the rotations are whatever the spec's reduction returns and the plain kernel runs
    (sbx_capi.hip tame_time): same operations as the model on whatever the matrices are"""
    for t in (3e8, -1e30, float("inf"), float("nan")):
        assert_same(renderer.render("egg_" + build, 64, 36, t), M.frame(build, 64, 36, t), (build, t))


@pytest.mark.parametrize("build", BUILDS)
def test_rows_host_rows_ranks_and_splits(renderer, build):
    import torch
    from shaderbox_amd import shard
    app = "egg_" + build
    w, h, br, t = 640, 360, 8, 0.2
    whole = renderer.render(app, w, h, t)
    assert_same(whole, model_frame(build, w, h, t), "whole")
    parts = [renderer.render(app, w, h, t, rows=(r0, r1)) for r0, r1 in [(0, 13), (13, 14), (14, 300), (300, h)]]
    assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32)), "rows"
    host = np.zeros((h, w, 4), dtype=np.float32)
    renderer.render_to_host(app, w, h, t, host)
    assert np.array_equal(host.view(np.uint32), whole.cpu().numpy().view(np.uint32)), "host rows"
    for n in (2, 3):
        for rr, rounds in [(1, 1), (1, 2)]:
            rows_max = shard.rank_rows_max(h, br, n, rr, rounds)
            gathered = torch.empty((n * rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
            for r in range(n):
                renderer.render_rank(app, w, h, t, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], root_rounds=rr, rounds=rounds)
            frame = renderer.assemble(gathered, w, h, br, n, root_rounds=rr, rounds=rounds)
            assert torch.equal(frame.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, "rank + assemble")
            for ch in (4, 3):
                inplace = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                if ch == 3:
                    inplace[..., 3] = 1.0
                for r in range(n):
                    renderer.render_rank_in_place(app, w, h, t, br, r, n, inplace, root_rounds=rr, rounds=rounds, channels=ch)
                assert torch.equal(inplace.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, ch, "in place")
            for ch in (4, 3):                                            # slab pieces, four channels and sbx_render_split_rgb
                slabs = torch.empty((n, rows_max, w, ch), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 0, 5, slabs[r], root_rounds=rr, rounds=rounds)
                    renderer.render_rank_rows(app, w, h, t, br, r, n, 5, rows_max, slabs[r], root_rounds=rr, rounds=rounds)
                root = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                renderer.render_rank_in_place(app, w, h, t, br, 0, n, root, root_rounds=rr, rounds=rounds)
                renderer.assemble_peers(slabs[1:].contiguous(), w, h, br, n, root, root_rounds=rr, rounds=rounds)
                assert torch.equal(root.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, ch, "peers")


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, build, n):
    """the span exchange (whole rows, as APP_EGG) and the direct exchange's rgb slabs, every rank's schedule on this GPU"""
    import torch
    from shaderbox_amd.distributed import LoopbackWorld
    app = "egg_" + build
    w, h, t = 1000, 333, 0.2
    full = renderer.render(app, w, h, t)
    for exchange, groups, relief in [("spans", 1, (1, 1)), ("spans", 2, (1, 2)), ("direct", 1, (1, 1))]:
        world = LoopbackWorld(n)
        plans = world.plans(renderer, w, h, block_rows=8, groups=groups, root_rounds=relief[0], rounds=relief[1], exchange=exchange)
        plans[0].frame.fill_(-7.0)
        got = LoopbackWorld.render(plans, app, t)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), full.view(torch.int32)), (n, exchange, groups, relief)


@pytest.mark.parametrize("build", BUILDS)
def test_span_table_gives_whole_rows(renderer, build):
    """sbx_span_table has no cost model for the scene: whole rows, as for APP_EGG"""
    w, h, t = 640, 360, 0.2
    table, pix, width = renderer.span_table("egg_" + build, w, h, t, 8, 2)
    ref = renderer.span_table("egg", w, h, t, 8, 2)
    assert (table[:, 0] == 0).all() and (table[:, 1] == w).all() and width == w
    assert np.array_equal(table, ref[0]) and np.array_equal(pix, ref[1]) and width == ref[2]


@pytest.mark.parametrize("build", BUILDS)
def test_rgba8_frames(renderer, build):
    app = "egg_" + build
    w, h, t = 800, 450, 0.2
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
    w, h, t = 257, 130, 0.2
    try:
        for build in BUILDS:
            renderer.set_precision("exact")
            a = renderer.render("egg_" + build, w, h, t).cpu().numpy()
            renderer.set_precision("1e-4")
            assert_same(renderer.render("egg_" + build, w, h, t), a, (build, "tier"))
    finally:
        renderer.set_precision("exact")


@pytest.mark.parametrize("build", BUILDS)
def test_multi_render(renderer, build):
    import torch
    import shaderbox_amd
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("sbx_multi_render across devices needs 2 or more visible GPUs (%d visible)" % ndev)
    w, h, t = 640, 360, 0.2
    m = shaderbox_amd.MultiRenderer(list(range(ndev)))
    try:
        got = m.render("egg_" + build, w, h, t)
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
    exe = str(tmp_path / ("APP_EGG_" + build.upper()))
    # -DAPP_EGG beside it, as a project that only adds the build's define would have: the build's define is tested first
    subprocess.run(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-DAPP_EGG", "-DAPP_EGG_" + build.upper(),
                    "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(rocm, "include"), "-o", exe, str(src), "-L" + lib, "-lsbx", "-L" + os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    for w, h, t in [(257, 130, 0.2), (96, 54, 0.0037)]:
        out = str(tmp_path / "px.f32")
        subprocess.run([exe, str(w), str(h), repr(t), out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
        assert_same(got, model_frame(build, w, h, t), ("dropin", build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    exe = os.path.join(ROOT, "host", "sbx_render")
    assert os.path.exists(exe), "host/sbx_render is built by build()"
    w, h = 257, 130
    for t in (0.2, -0.41):
        out = str(tmp_path / "frame.f32")
        subprocess.run([exe, "--app", "egg_" + build, "--res", "%dx%d" % (w, h), "--time", repr(t), "--f32", out], check=True, timeout=120)
        raw = np.fromfile(out, dtype=np.float32)
        assert raw.size == w * h * 4
        assert_same(raw.reshape(h, w, 4), model_frame(build, w, h, t), ("sbx_render --app egg_" + build, t))
