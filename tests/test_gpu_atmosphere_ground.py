"""GPU tests of SBX_APP_ATMOSPHERE_GROUND (src/app_atmosphere.h without FROM_SPACE; include/sbx.h): every layer bit for bit,
NaN == NaN, all four channels, against tests/atmosphere_ground_model.py (numpy camera and plane test over the oracle's
get_incident_light).  Frames above 320x180 are compared by point samples, or GPU against GPU (plain kernel, tier)."""
import os
import subprocess

import numpy as np
import pytest

from tests import atmosphere_ground_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APP = "atmosphere_ground"
TIMES = (0.0, .37, 2.0, 3.1, 100.25)
F = np.float32


@pytest.fixture(scope="module")
def renderer():
    import shaderbox_amd
    r = shaderbox_amd.Renderer(0)
    yield r
    r.close()


_FRAMES = {}


def model_frame(w, h, t):
    if (w, h, t) not in _FRAMES:
        _FRAMES[(w, h, t)] = M.frame(w, h, t)
    return _FRAMES[(w, h, t)]


def assert_same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = M.same_bits(got, want)
    if not ok.all():
        i = np.argwhere(~ok)[:3]
        raise AssertionError("%s: %d differing channels, first %s: got %s want %s"
                             % (what, int((~ok).sum()), i.tolist(), [got[tuple(j)] for j in i], [want[tuple(j)] for j in i]))


def same_tensor(a, b, what):
    import torch
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9), (257, 2), (96, 54), (320, 180)])
def test_frames(renderer, w, h):
    for t in TIMES:
        want = model_frame(w, h, t)
        assert (want[..., 3] == 1).all()
        assert_same(renderer.render(APP, w, h, t), want, (w, h, t))
    assert_same(renderer.render(APP, w, h, .37, mouse=(50.0, 60.0)), model_frame(w, h, .37), "u_mouse does not enter")


def _horizon_band(w, h, n=300):
    """consecutive binary32 fragCoord.y values either side of the place where the model's plane test flips from ground to sky
    (denom = 1e-6) and on down past denom = 0 (ny ~ .2205)"""
    lo, hi = F(.21 * h), F(.23 * h)                                  # ground at lo, sky at hi

    def sky(fy):
        pcx, pcy = M.point_cam(w, h, F(w / 2), fy)
        return bool(M.intersect_plane_t(M.get_primary_ray(pcx, pcy, M.EYE, M.LOOK_AT)) > M.MAX_DIST)
    assert not sky(lo) and sky(hi)
    while np.nextafter(lo, hi) < hi:
        mid = F((np.float64(lo) + np.float64(hi)) / 2)
        lo, hi = (lo, mid) if sky(mid) else (mid, hi)
    ys = [hi]
    for _ in range(n):
        ys.append(np.nextafter(ys[-1], F(np.inf)))
    down = [lo]
    for _ in range(n):
        down.append(np.nextafter(down[-1], F(-np.inf)))
    ys = np.array(down[::-1] + ys, dtype=F)
    xs = np.resize(np.array([.5, w / 2, w - .5, w / 3, -2.0 * w, 3.0 * w], dtype=F), len(ys))
    return np.stack([xs, ys], axis=-1)


def _points(w, h):
    rng = np.random.default_rng(16)
    return np.concatenate([
        rng.uniform(0, 1, size=(300, 2)) * [w, h],                      # off-centre
        rng.uniform(-3, 4, size=(200, 2)) * [w, h],                     # outside the frame
        _horizon_band(w, h),                                            # both sides of denom = 1e-6
        np.stack([rng.uniform(0, w, 200), rng.uniform(.2204, .2206, 200) * h], axis=-1),
        [[w / 2, 1.5 * h], [w / 2 + .25, 1.5 * h], [w / 2, 40.0 * h], [0, 0], [w, h], [-.5, -.5]],   # straight up, far up, corners
        [[1e30, 1e30], [-3e38, 5], [3e38, -3e38], [5, 3e38], [1e19 * w, 1e19 * h], [3e19 * w, .3 * h], [1e12, 1e12]],   # |v|^2 overflows
        [[np.inf, 5], [5, -np.inf], [5, np.inf], [np.inf, np.inf], [np.nan, 5], [5, np.nan], [np.nan, np.nan], [np.inf, np.nan]],
    ]).astype(F)


@pytest.mark.parametrize("w,h", [(1920, 1080), (7680, 4320)])
def test_points_and_main_image(renderer, w, h, oracle):
    import torch
    pts = _points(w, h)
    t = 2.0
    want = M.main_image(w, h, t, pts[:, 0], pts[:, 1])
    grey = oracle.math("pow", np.array([.33], dtype=F), F(1) / F(2.2))[0]
    is_grey = (want[:, :3] == grey).all(axis=-1)
    assert is_grey[-4:].all(), "a NaN direction is a ground hit"
    band = slice(500, 500 + 602)
    assert is_grey[band].any() and (~is_grey[band]).any()
    got = renderer.render_points(APP, w, h, t, torch.from_numpy(pts))
    assert_same(got, want, "points")
    idx = np.r_[0:40, 780:820, len(pts) - 21:len(pts)]
    assert_same(renderer.main_image_batch(APP, w, h, t, pts[idx]), want[idx], "batch")
    for i in [0, 1, 301, 790, 801, 802, len(pts) - 1, len(pts) - 8, len(pts) - 15, len(pts) - 21]:
        c = renderer.main_image(APP, w, h, t, (float(pts[i, 0]), float(pts[i, 1])))
        assert_same(np.asarray(c, dtype=F), want[i], ("main_image", i))
    if w == 1920:                                                      # pixel centres: served from the cached frame
        for x, y in [(10, 20), (960, 238), (960, 239), (1900, 1079)]:
            c = renderer.main_image(APP, w, h, t, (x + .5, y + .5))
            assert_same(np.asarray(c, dtype=F), M.main_image(w, h, t, F(x + .5), F(y + .5)), ("centre", x, y))


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160)])
def test_plain_variant_same_bits(renderer, w, h):
    """sbx_set_variant(1): the plain kernel.  Every pixel of the full frames and of the point set."""
    import torch
    pts = torch.from_numpy(_points(w, h))
    for t in (.37, 2.0):
        try:
            renderer.set_variant(0)
            a, pa = renderer.render(APP, w, h, t), renderer.render_points(APP, w, h, t, pts)
            renderer.set_variant(1)
            b, pb = renderer.render(APP, w, h, t), renderer.render_points(APP, w, h, t, pts)
        finally:
            renderer.set_variant(0)
        assert_same(a, b.cpu().numpy(), ("frame variant 0 vs 1", w, h, t))
        assert_same(pa, pb.cpu().numpy(), ("points variant 0 vs 1", w, h, t))
    rows = [0, M.horizon_row(w, h) - 1, M.horizon_row(w, h), h // 2, h - 1]
    xs = np.arange(0, w, 97)
    want = M.main_image(w, h, 2.0, (xs + .5).astype(F)[None, :], (np.array(rows) + .5).astype(F)[:, None])
    assert_same(a.cpu().numpy()[rows][:, xs], want, "samples of the large frame vs the model")


def test_precision_tier_within_1e4(renderer):
    """SBX_PRECISION_1E4 against the exact frame of the same build: max |tier - exact| over EVERY pixel of 3840x2160 at each u_time
    must be <= 1e-4 (BASELINE.json's bar, quoted by include/sbx.h).  Measured on MI355X: 4.8e-7 at worst (u_time 2 and 3.1;
    profiles/atmosphere_ground_timing.txt).  The plain variant stays exact under the tier."""
    import torch
    w, h = 3840, 2160
    worst = 0.0
    try:
        for t in TIMES:
            renderer.set_precision("exact")
            exact = renderer.render(APP, w, h, t)
            renderer.set_precision("1e-4")
            tier = renderer.render(APP, w, h, t)
            assert bool(torch.isfinite(exact).all()) and bool(torch.isfinite(tier).all())
            d = float((tier - exact).abs().max())
            print("atmosphere_ground tier: u_time %-7g max |tier - exact| = %.3e   (max channel %.3f)" % (t, d, float(exact[..., :3].max())))
            worst = max(worst, d)
            hz = M.horizon_row(w, h)
            same_tensor(tier[:hz], exact[:hz], "ground rows are exact under the tier")
            assert d > 0, "the tier kernel did not run"
            renderer.set_variant(1)
            same_tensor(renderer.render(APP, w, h, t), exact, "variant 1 is exact whatever the tier")
            renderer.set_variant(0)
        assert worst <= 1e-4, worst
    finally:
        renderer.set_variant(0)
        renderer.set_precision("exact")


def test_non_finite_uniforms(renderer):
    import torch
    w, h = 96, 54
    for t in (float("nan"), float("inf"), -float("inf")):
        sun = M.sun_dir(t)
        assert np.isnan(sun).any()
        want = model_frame(w, h, t)
        assert_same(renderer.render(APP, w, h, t), want, ("u_time", t))
    # sbx_render_points takes any positive finite u_res: one whose aspect ratio overflows makes the camera non-finite (plain kernel)
    import shaderbox_amd
    pts = torch.tensor([[1.5e38, 40.5], [3.0, 2.0], [2e38, 5e-4], [float("nan"), 1.0]], dtype=torch.float32)
    for res in [(3e38, 1e-3), (3e38, 3e38), (1e-3, 3e38)]:
        want = M.main_image(res[0], res[1], .37, pts[:, 0].numpy(), pts[:, 1].numpy())
        assert_same(renderer.render_points(APP, res[0], res[1], .37, pts), want, ("u_res", res))
    for res in [(float("inf"), 54.0), (96.0, float("nan"))]:           # refused before any launch, as for every app
        with pytest.raises(shaderbox_amd.SbxError):
            renderer.render_points(APP, res[0], res[1], .37, pts)


def test_rows_host_rows_ranks_and_splits(renderer):
    import torch
    from shaderbox_amd import shard
    w, h, br, t = 320, 180, 8, 2.0
    whole = renderer.render(APP, w, h, t)
    assert_same(whole, model_frame(w, h, t), "whole")
    parts = [renderer.render(APP, w, h, t, rows=(a, b)) for a, b in [(0, 13), (13, 39), (39, 40), (40, 41), (41, h)]]
    same_tensor(torch.cat(parts), whole, "rows")
    host = np.zeros((h, w, 4), dtype=F)
    renderer.render_to_host(APP, w, h, t, host)
    assert np.array_equal(host.view(np.uint32), whole.cpu().numpy().view(np.uint32)), "host rows"
    for n in (2, 3):
        for rr, rounds in [(1, 1), (1, 2)]:
            rows_max = shard.rank_rows_max(h, br, n, rr, rounds)
            gathered = torch.empty((n * rows_max, w, 4), dtype=torch.float32, device=renderer.tdev)
            for r in range(n):
                renderer.render_rank(APP, w, h, t, br, r, n, out=gathered[r * rows_max:(r + 1) * rows_max], root_rounds=rr, rounds=rounds)
            frame = renderer.assemble(gathered, w, h, br, n, root_rounds=rr, rounds=rounds)
            same_tensor(frame, whole, (n, rr, rounds, "rank + assemble"))
            for ch in (4, 3):
                inplace = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                if ch == 3:
                    inplace[..., 3] = 1.0
                for r in range(n):
                    renderer.render_rank_in_place(APP, w, h, t, br, r, n, inplace, root_rounds=rr, rounds=rounds, channels=ch)
                same_tensor(inplace, whole, (n, rr, rounds, ch, "in place"))
            for ch in (4, 3):                                            # slab pieces, four channels and sbx_render_split_rgb
                slabs = torch.empty((n, rows_max, w, ch), dtype=torch.float32, device=renderer.tdev)
                for r in range(n):
                    renderer.render_rank_rows(APP, w, h, t, br, r, n, 0, 5, slabs[r], root_rounds=rr, rounds=rounds)
                    renderer.render_rank_rows(APP, w, h, t, br, r, n, 5, rows_max, slabs[r], root_rounds=rr, rounds=rounds)
                root = torch.full((h, w, 4), float("nan"), device=renderer.tdev)
                renderer.render_rank_in_place(APP, w, h, t, br, 0, n, root, root_rounds=rr, rounds=rounds)
                renderer.assemble_peers(slabs[1:].contiguous(), w, h, br, n, root, root_rounds=rr, rounds=rounds)
                same_tensor(root, whole, (n, rr, rounds, ch, "peers"))


@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, n):
    """the span exchange (peer + root + assemble; only sky blocks carry spans) and the direct exchange's rgb slabs, every rank's
    schedule on this GPU"""
    import torch
    from shaderbox_amd.distributed import LoopbackWorld
    w, h, t = 1000, 333, 2.0
    full = renderer.render(APP, w, h, t)
    for exchange, groups, relief in [("spans", 1, (1, 1)), ("spans", 2, (1, 2)), ("direct", 1, (1, 1))]:
        world = LoopbackWorld(n)
        plans = world.plans(renderer, w, h, block_rows=8, groups=groups, root_rounds=relief[0], rounds=relief[1], exchange=exchange)
        plans[0].frame.fill_(-7.0)
        got = LoopbackWorld.render(plans, APP, t)
        torch.cuda.synchronize()
        same_tensor(got, full, (n, exchange, groups, relief))


@pytest.mark.parametrize("nranks", [2, 4])
def test_multi_renderer_on_one_device(renderer, nranks):
    """sbx_multi_render with every rank on device 0, every exchange: the one-launch frame"""
    import torch
    import shaderbox_amd
    m = shaderbox_amd.MultiRenderer([0] * nranks)
    try:
        for exchange in ("slabs", "blocks", "spans"):
            m.set_exchange(exchange)
            for (w, h, t), split in [((1000, 333, 2.0), (8, 1, 1)), ((1111, 500, .37), (8, 1, 2))]:
                m.set_split(*split)
                got = m.render(APP, w, h, t)
                torch.cuda.synchronize()
                same_tensor(got, renderer.render(APP, w, h, t), (exchange, w, h, t, nranks, split))
    finally:
        m.close()


def test_rgba8_frames(renderer):
    w, h, t = 800, 450, 2.0
    try:
        renderer.set_output_format("rgba32f")
        f = renderer.render(APP, w, h, t)
        assert float(f[..., :3].max()) > 1.0                            # channels above 1 clamp to 255
        packed = renderer.pack_unorm8(f, flip_y=False)
        renderer.set_output_format("rgba8")
        got = renderer.render(APP, w, h, t)
        assert np.array_equal(got.cpu().numpy(), packed.cpu().numpy())
        assert (got.cpu().numpy()[..., 3] == 255).all()
    finally:
        renderer.set_output_format("rgba32f")


def test_dome_build_untouched_on_the_same_context(renderer, oracle):
    """SBX_APP_ATMOSPHERE still equals the oracle after renders of the new app on the same context (tier and variant toggled)"""
    from oracle.oracle import APP_ATMOSPHERE
    w, h, t = 640, 360, .37
    renderer.render(APP, w, h, t)
    renderer.set_variant(1)
    renderer.render(APP, w, h, t)
    renderer.set_variant(0)
    got = renderer.render("atmosphere", w, h, t)
    renderer.render(APP, w, h, t)
    assert_same(got, oracle.render(APP_ATMOSPHERE, w, h, t), "dome build vs oracle")
    assert_same(renderer.render("planet_atmosphere", 160, 90, t), oracle.render(12, 160, 90, t), "planet composite vs oracle")


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
    exe = str(tmp_path / "APP_ATMOSPHERE_GROUND")
    subprocess.run(["g++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-DAPP_ATMOSPHERE_GROUND", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(rocm, "include"), "-o", exe, str(src), "-L" + lib, "-lsbx", "-L" + os.path.join(rocm, "lib"),
                    "-lamdhip64", "-Wl,-rpath," + lib, "-Wl,-rpath," + os.path.join(rocm, "lib")], check=True)
    for w, h, t in [(96, 54, 0.37), (33, 9, 2.0)]:
        out = str(tmp_path / "px.f32")
        subprocess.run([exe, str(w), str(h), repr(t), out], check=True, timeout=120)
        got = np.fromfile(out, dtype=F).reshape(h, w, 4)
        assert_same(got, model_frame(w, h, t), ("dropin", w, h, t))


def test_mainimage_demo_through_the_host_makefile(tmp_path):
    """host/Makefile's drop-in demo built with APP=-DAPP_ATMOSPHERE_GROUND (in a copy of host/, so the tree's binaries stay)"""
    import shutil
    host = tmp_path / "host"
    shutil.copytree(os.path.join(ROOT, "host"), host, ignore=shutil.ignore_patterns("sbx_render", "mainimage_demo", "mainimage_threads",
                                                                                   "mainimage_stress", "inclxpnd", "sbx_ddsvolgen"))
    os.symlink(os.path.join(ROOT, "include"), tmp_path / "include")
    os.symlink(os.path.join(ROOT, "shaderbox_amd"), tmp_path / "shaderbox_amd")
    subprocess.run(["make", "-s", "-C", str(host), "mainimage_demo", "APP=-DAPP_ATMOSPHERE_GROUND"], check=True)
    r = subprocess.run([str(host / "mainimage_demo"), "96", "54", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    mean = [float(v) for v in r.stdout.strip().split("=")[-1].split()]
    want = model_frame(96, 54, 2.0)[..., :3].astype(np.float64).reshape(-1, 3).mean(axis=0)
    assert np.allclose(mean, want, atol=2e-6), (r.stdout, want)


def test_sbx_render_host(tmp_path):
    exe = os.path.join(ROOT, "host", "sbx_render")
    assert os.path.exists(exe), "host/sbx_render is built by build()"
    w, h, t = 257, 130, 2.0
    out = str(tmp_path / "ground.f32")
    subprocess.run([exe, "--app", APP, "--res", "%dx%d" % (w, h), "--time", repr(t), "--f32", out], check=True, timeout=120)
    raw = np.fromfile(out, dtype=F)
    assert raw.size >= w * h * 4
    got = raw[-w * h * 4:].reshape(h, w, 4)
    assert_same(got, model_frame(w, h, t), "sbx_render --app atmosphere_ground")
