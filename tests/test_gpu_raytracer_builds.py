"""GPU tests of SBX_APP_RAYTRACER_PHONG, SBX_APP_RAYTRACER_NOSHADOW and SBX_APP_RAYTRACER_STATIC (src/app_raytracer.h with its `#if 0`
at :61 on / its `#if 1` at :107 off / its `#if 1` at :29 off; include/sbx.h): every layer bit for bit, NaN == NaN,
all four channels, against the frames and points the edited reference header rendered (tests/golden/raytracer_builds/) and against
tests/raytracer_builds_model.py."""
import os

import numpy as np
import pytest

from tests import raytracer_builds_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["phong", "noshadow", "static"]
W, H, T = 64, 64, 0.37                                                  # the layer checks' frame

model_frame = frame_cache(lambda build, w, h, t, mouse=(0.0, 0.0): M.frame(build, w, h, t, mouse))


@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames_and_points(renderer, build):
    """what src/app_raytracer.h itself rendered with the one line edited, from the default kernel and the IEEE six-plane one"""
    import torch
    fx = M.fixture(build)
    pts, u = fx["points"], fx["points_uniforms"]
    try:
        for variant in (0, 1):
            renderer.set_variant(variant)
            for w, h, t, mouse, want in fx["frames"]:
                assert_same(renderer.render(M.APP_OF[build], w, h, t, mouse=mouse), want, (build, t, mouse, "variant", variant))
            got = renderer.render_points(M.APP_OF[build], int(u[0]), int(u[1]), float(u[4]), torch.from_numpy(pts))
            assert_same(got, fx["points_out"], (build, "points", "variant", variant))
    finally:
        renderer.set_variant(0)


@pytest.mark.parametrize("build", BUILDS)
def test_frame_whose_width_is_no_multiple_of_the_tile(renderer, build):
    w, h = 97, 55
    for t, mouse in [(1.5, (0.0, 0.0)), (-3.7, (70.0, 3.0))]:
        assert_same(renderer.render(M.APP_OF[build], w, h, t, mouse=mouse), model_frame(build, w, h, t, mouse), (build, w, h, t, mouse))


def _uniform_sets(build):
    """six seeded (u_time, u_mouse), three of them with the camera turned; u_time inf and NaN where the build reads it (the frame
    block goes non-finite and hit_walls stands down)"""
    rng = np.random.default_rng(29)
    sets = [(float(t), (0.0, 0.0)) for t in rng.uniform(-20, 20, size=3)]
    sets += [(float(t), (float(mx), float(my))) for t, mx, my in zip(rng.uniform(-20, 20, size=3), rng.uniform(20, 256, size=3), rng.uniform(1, 144, size=3))]
    if build != "static":
        sets += [(float("inf"), (0.0, 0.0)), (float("nan"), (120.0, 30.0))]
    return sets


@pytest.mark.parametrize("build", BUILDS)
def test_default_witness_edge_and_ieee_kernels_agree(renderer, build):
    w, h = 256, 144
    app = M.APP_OF[build]
    try:
        for t, mouse in _uniform_sets(build):
            got = {}
            for v in (0, 1, 2, 3):
                renderer.set_variant(v)
                got[v] = renderer.render(app, w, h, t, mouse=mouse).cpu().numpy()
            for v in (1, 2, 3):
                assert_same(got[v], got[0], (build, t, mouse, "variant 0 vs", v))
            assert (got[0][..., 3] == 1).all()
            renderer.set_variant(0)
            shipped = renderer.render("raytracer", w, h, t, mouse=mouse).cpu().numpy()
            assert not M.same_bits(got[0], shipped).all(), (build, t, mouse, "the shipped build's frame")
    finally:
        renderer.set_variant(0)


def test_static_build_reads_no_time(renderer):
    want = renderer.render("raytracer_static", W, H, 0.0).cpu().numpy()
    assert_same(want, model_frame("static", W, H, 0.0), "static")
    for t in (7.25, float("nan")):
        assert_same(renderer.render("raytracer_static", W, H, t), want, ("static", t))


def test_pow_is_its_statement_at_exponent_50(renderer):
    """phong()'s pow_(x, 50.f) against pow_spec_ on all 2^32 arguments (the loop of tests/test_gpu_round3.py
    test_pow_equals_its_statement at the one exponent that kernel adds)"""
    import torch
    chunk = 1 << 26
    for start in range(0, 1 << 32, chunk):
        x = torch.arange(start, start + chunk, dtype=torch.int64, device="cuda").to(torch.int32).view(torch.float32)
        yy = torch.full_like(x, 50.0)
        a, b = renderer.math("pow", x, yy), renderer.math("pow_spec", x, yy)
        bad = (a.view(torch.int32) != b.view(torch.int32)) & ~(torch.isnan(a) & torch.isnan(b))
        assert not bool(bad.any()), float(x[bad][0])


@pytest.mark.parametrize("build", BUILDS)
def test_rows_host_rows_ranks_and_splits(renderer, build):
    check_rows_host_rows_ranks_and_splits(renderer, M.APP_OF[build], W, H, T, model_frame(build, W, H, T), cuts=[13, 14, 40], block_rows=8)


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, build, n):
    check_loopback_exchanges(renderer, M.APP_OF[build], n, W, H, T)


@pytest.mark.parametrize("build", BUILDS)
def test_rgba8_frames(renderer, build):
    check_rgba8(renderer, M.APP_OF[build], W, H, T)


@pytest.mark.parametrize("build", BUILDS)
def test_multi_render(renderer, build):
    check_multi_render(M.APP_OF[build], W, H, T, lambda: model_frame(build, W, H, T))


@pytest.mark.parametrize("build", BUILDS)
def test_cpp_dropin(tmp_path, build):
    # -DAPP_RAYTRACER beside it, as a project that only adds the build's define would have: the build's define is tested first
    exe = build_dropin(tmp_path, ["APP_RAYTRACER", "APP_RAYTRACER_" + build.upper()], "APP_RAYTRACER_" + build.upper())
    assert_same(run_dropin(exe, W, H, T, tmp_path), model_frame(build, W, H, T), ("dropin", build))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    assert_same(run_sbx_render(tmp_path, M.APP_OF[build], W, H, T), model_frame(build, W, H, T), ("sbx_render --app " + M.APP_OF[build],))


def test_shipped_build_between_and_after_the_new_apps(renderer):
    """one context, the apps taking turns: SBX_APP_RAYTRACER keeps returning its own golden frame"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "raytracer_64x64.npz"))
    for key in ("t0.37", "t2.5"):
        t = float(key[1:])
        for build in BUILDS:
            assert_same(renderer.render(M.APP_OF[build], 64, 64, t), model_frame(build, 64, 64, t), (build, "in turn", t))
            assert_same(renderer.render("raytracer", 64, 64, t), z[key], ("raytracer after", build, t))
