"""GPU tests of SBX_APP_FUNC (src/app_func.h's 2D branch; include/sbx.h): every layer bit for bit, NaN == NaN, all four channels,
against the restatement of tests/appfunc_model.py (oracle noise_w, binary32 combination)."""
import os
import subprocess

import numpy as np
import pytest

from tests import appfunc_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def renderer():
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


_FRAMES = {}


def model_frame(w, h):
    if (w, h) not in _FRAMES:
        _FRAMES[(w, h)] = M.frame(w, h)
    return _FRAMES[(w, h)]


def assert_same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = M.same_bits(got, want)
    if not ok.all():
        i = np.argwhere(~ok)[:3]
        raise AssertionError("%s: %d differing channels, first %s: got %s want %s"
                             % (what, int((~ok).sum()), i.tolist(), [got[tuple(j)] for j in i], [want[tuple(j)] for j in i]))


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9), (257, 2), (640, 360), (1920, 1080)])
def test_frames(renderer, w, h):
    want = model_frame(w, h)
    assert (want[..., 3] == 1).all()
    for t, mouse in [(0.37, (0.0, 0.0)), (123.25, (50.0, 60.0)), (-7.0, (-3.0, 1e6))]:    # u_time and u_mouse do not enter
        assert_same(renderer.render("func", w, h, t, mouse=mouse), want, (w, h, t, mouse))


def _points(w, h):
    rng = np.random.default_rng(11)
    big = float(2 ** 24) * w
    return np.concatenate([
        rng.uniform(0, 1, size=(400, 2)) * [w, h],                      # off-centre
        rng.uniform(-3, 4, size=(300, 2)) * [w, h],                     # negative and outside the frame
        rng.uniform(-1, 1, size=(50, 2)) * [big, big * 16],             # beyond 2^24 W: mod's quotient rounds
        [[0, 0], [w, h], [-.5, -.5], [w - .5, h - .5], [-1, 7], [big, 3], [3, -big], [1e30, 1e30], [-3e38, 5], [3e38, -3e38]],
        [[np.inf, 5], [5, -np.inf], [np.inf, np.inf], [np.nan, 5], [5, np.nan], [np.nan, np.nan], [np.inf, np.nan]],
    ]).astype(np.float32)


def test_points_and_main_image(renderer):
    import torch
    w, h = 1920, 1080
    pts = _points(w, h)
    want = M.main_image(w, h, pts[:, 0], pts[:, 1])
    nan_row = np.float32(1) - (np.float32(10) + np.float32(.015))        # F1 stays 100 for every period
    assert (want[-4:, 0] == nan_row).all()
    got = renderer.render_points("func", w, h, 0.37, torch.from_numpy(pts))
    assert_same(got, want, "points")
    batch = renderer.main_image_batch("func", w, h, 0.37, pts[:64])
    assert_same(batch, want[:64], "batch")
    for i in [0, 1, 400, 701, 750, 755, len(pts) - 1, len(pts) - 4]:
        c = renderer.main_image("func", w, h, 0.37, (float(pts[i, 0]), float(pts[i, 1])))
        assert_same(np.asarray(c, dtype=np.float32), want[i], ("main_image", i))
    c = renderer.main_image("func", w, h, 0.37, (10.5, 20.5))          # a pixel centre: served from the cached frame
    assert_same(np.asarray(c, dtype=np.float32), model_frame(w, h)[20, 10], "centre")


def test_plain_variant_same_bits(renderer):
    import torch
    w, h = 1920, 1080
    pts = torch.from_numpy(_points(w, h))
    try:
        renderer.set_variant(0)
        a, pa = renderer.render("func", w, h, 0.37), renderer.render_points("func", w, h, 0.37, pts)
        renderer.set_variant(1)
        b, pb = renderer.render("func", w, h, 0.37), renderer.render_points("func", w, h, 0.37, pts)
    finally:
        renderer.set_variant(0)
    assert_same(a, b.cpu().numpy(), "frame variant 0 vs 1")
    assert_same(pa, pb.cpu().numpy(), "points variant 0 vs 1")
    assert_same(a, model_frame(w, h), "frame vs model")


def test_noise_eval_worley_fbm(renderer):
    import torch
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.uniform(-2, 3, size=(3000, 3)), rng.uniform(0, 1, size=(1000, 3)) * [1, 1, 0],
                          [[np.nan, 0, 0], [np.inf, .5, 0], [1e9, -1e9, 3]]]).astype(np.float32)
    got = renderer.noise("worley_fbm", torch.from_numpy(xyz)).cpu().numpy()[:, 0]
    assert_same(got, M.worley_fbm_xyz(xyz), "worley_fbm")


def test_rows_host_rows_ranks_and_splits(renderer):
    import torch
    from shaderbox_amd import shard
    w, h, br = 640, 360, 8
    whole = renderer.render("func", w, h, 0.37)
    assert_same(whole, model_frame(w, h), "whole")
    parts = [renderer.render("func", w, h, 0.37, rows=(a, b)) for a, b in [(0, 13), (13, 14), (14, 300), (300, h)]]
    assert torch.equal(torch.cat(parts).view(torch.int32), whole.view(torch.int32)), "rows"
    host = np.zeros((h, w, 4), dtype=np.float32)
    renderer.render_to_host("func", w, h, 0.37, host)
    assert np.array_equal(host.view(np.uint32), whole.cpu().numpy().view(np.uint32)), "host rows"
    for n in (2, 3):
        for rr, rounds in [(1, 1), (1, 2)]:
            rows_max = shard.rank_rows_max(h, br, n, rr, rounds)
            gathered = torch.empty((n * rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
            for r in range(n):
                renderer.render_rank("func", w, h, 0.37, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], root_rounds=rr, rounds=rounds)
            frame = renderer.assemble(gathered, w, h, br, n, root_rounds=rr, rounds=rounds)
            assert torch.equal(frame.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, "rank + assemble")
            for ch in (4, 3):
                inplace = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                if ch == 3:
                    inplace[..., 3] = 1.0
                for r in range(n):
                    renderer.render_rank_in_place("func", w, h, 0.37, br, r, n, inplace, root_rounds=rr, rounds=rounds, channels=ch)
                assert torch.equal(inplace.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, ch, "in place")
            for ch in (4, 3):                                            # slab pieces, four channels and sbx_render_split_rgb
                slabs = torch.empty((n, rows_max, w, ch), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_rows("func", w, h, 0.37, br, r, n, 0, 5, slabs[r], root_rounds=rr, rounds=rounds)
                    renderer.render_rank_rows("func", w, h, 0.37, br, r, n, 5, rows_max, slabs[r], root_rounds=rr, rounds=rounds)
                root = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                renderer.render_rank_in_place("func", w, h, 0.37, br, 0, n, root, root_rounds=rr, rounds=rounds)
                renderer.assemble_peers(slabs[1:].contiguous(), w, h, br, n, root, root_rounds=rr, rounds=rounds)
                assert torch.equal(root.view(torch.int32), whole.view(torch.int32)), (n, rr, rounds, ch, "peers")


@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, n):
    """the span exchange (whole rows: no cost model) and the direct exchange's rgb slabs, every rank's schedule on this GPU"""
    import torch
    from shaderbox_amd.distributed import LoopbackWorld
    w, h = 1000, 333
    full = renderer.render("func", w, h, 0.37)
    for exchange, groups, relief in [("spans", 1, (1, 1)), ("spans", 2, (1, 2)), ("direct", 1, (1, 1))]:
        world = LoopbackWorld(n)
        plans = world.plans(renderer, w, h, block_rows=8, groups=groups, root_rounds=relief[0], rounds=relief[1], exchange=exchange)
        plans[0].frame.fill_(-7.0)
        got = LoopbackWorld.render(plans, "func", 0.37)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), full.view(torch.int32)), (n, exchange, groups, relief)


def test_rgba8_frames(renderer):
    w, h = 800, 450
    try:
        renderer.set_output_format("rgba32f")
        f = renderer.render("func", w, h, 0.37)
        packed = renderer.pack_unorm8(f, flip_y=False)
        renderer.set_output_format("rgba8")
        got = renderer.render("func", w, h, 0.37)
        assert np.array_equal(got.cpu().numpy(), packed.cpu().numpy())
        assert (got.cpu().numpy()[..., 3] == 255).all()
    finally:
        renderer.set_output_format("rgba32f")


def test_multi_render(renderer):
    import torch
    import shaderbox_amd
    ndev = torch.cuda.device_count()
    if ndev < 2:
        pytest.skip("sbx_multi_render across devices needs 2 or more visible GPUs (%d visible)" % ndev)
    w, h = 1280, 720
    m = shaderbox_amd.MultiRenderer(list(range(ndev)))
    try:
        got = m.render("func", w, h, 0.37)
        torch.cuda.synchronize()
        assert_same(got, model_frame(w, h), "multi")
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


def test_cpp_dropin(tmp_path):
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    src = tmp_path / "dropin.cpp"
    src.write_text(DROPIN)
    lib = os.path.join(ROOT, "shaderbox_amd", "lib")
    exe = str(tmp_path / "APP_FUNC")
    subprocess.run(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-DAPP_FUNC", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(rocm, "include"), "-o", exe, str(src), "-L" + lib, "-lsbx", "-L" + os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    for w, h, t in [(320, 180, 0.37), (97, 61, 9.25)]:
        out = str(tmp_path / "px.f32")
        subprocess.run([exe, str(w), str(h), repr(t), out], check=True, timeout=120)
        got = np.fromfile(out, dtype=np.float32).reshape(h, w, 4)
        assert_same(got, model_frame(w, h), ("dropin", w, h, t))


def test_sbx_render_host(tmp_path):
    exe = os.path.join(ROOT, "host", "sbx_render")
    assert os.path.exists(exe), "host/sbx_render is built by build()"
    w, h = 257, 130
    out = str(tmp_path / "func.f32")
    subprocess.run([exe, "--app", "func", "--res", "%dx%d" % (w, h), "--time", "0.37", "--f32", out], check=True, timeout=120)
    raw = np.fromfile(out, dtype=np.float32)
    assert raw.size >= w * h * 4
    got = raw[-w * h * 4:].reshape(h, w, 4)
    assert_same(got, model_frame(w, h), "sbx_render --app func")
