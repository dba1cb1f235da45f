"""GPU tests of SBX_APP_VINYL_CLOSEUP, SBX_APP_VINYL_RIDGES and SBX_APP_VINYL_NOSHADOW (src/app_vinyl.h with its `#if 1` at :60 off /
its `#if 0` at :357 on / its `#if 1` at :445 off; include/sbx.h): every layer bit for bit, NaN == NaN, all four
channels, against the frames and points the edited reference header rendered (tests/golden/vinyl_builds/) and against
tests/vinyl_builds_model.py."""
import os

import numpy as np
import pytest

from tests import vinyl_builds_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["closeup", "ridges", "noshadow"]
W, H, T = 64, 36, 2.5                                                   # the layer checks' frame


def _model(build, w, h, t):
    parts = {}
    return (M.frame(build, w, h, t, parts=parts), parts)


model = frame_cache(_model)


def model_frame(build, w, h, t):
    return model(build, w, h, t)[0]


@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames_and_points(renderer, build):
    """what src/app_vinyl.h itself rendered with the one line edited, from the default kernel and the plain one"""
    import torch
    fx = M.fixture(build)
    pts, u = fx["points"], fx["points_uniforms"]
    try:
        for variant in (0, 1):
            renderer.set_variant(variant)
            for uni, want in list(zip(fx["uniforms"], fx["frames"])) + list(zip(fx["big_uniforms"], fx["big_frames"])):
                w, h, t = int(uni[0]), int(uni[1]), float(uni[4])
                assert_same(renderer.render(M.APP_OF[build], w, h, t), want, (build, w, h, t, "variant", variant))
            got = renderer.render_points(M.APP_OF[build], int(u[0]), int(u[1]), float(u[4]), torch.from_numpy(pts))
            assert_same(got, fx["points_out"], (build, "points", "variant", variant))
    finally:
        renderer.set_variant(0)


@pytest.mark.parametrize("build", BUILDS)
def test_frame_whose_width_is_no_multiple_of_the_tile(renderer, build):
    w, h = 97, 55
    for t in (2.5, -3.7):
        assert_same(renderer.render(M.APP_OF[build], w, h, t), model_frame(build, w, h, t), (build, w, h, t))


def _times():
    """six seeded u_time; inf and NaN, which tame_time sends to the plain kernels whatever the variant; 2e8, beyond tame_time"""
    rng = np.random.default_rng(31)
    return [float(t) for t in rng.uniform(-20, 20, size=6)] + [float("inf"), float("nan"), 2e8]


@pytest.mark.parametrize("build", BUILDS)
def test_default_plain_witness_edge_and_ieee_kernels_agree(renderer, build):
    w, h = 256, 144
    app = M.APP_OF[build]
    try:
        for t in _times():
            got = {}
            for v in (0, 1, 2, 3):
                renderer.set_variant(v)
                got[v] = renderer.render(app, w, h, t).cpu().numpy()
            for v in (1, 2, 3):
                assert_same(got[v], got[0], (build, t, "variant 0 vs", v))
            assert (got[0][..., 3] == 1).all()
            renderer.set_variant(0)
            if np.isfinite(t):
                shipped = renderer.render("vinyl", w, h, t).cpu().numpy()
                assert not M.same_bits(got[0], shipped).all(), (build, t, "the shipped build's frame")
    finally:
        renderer.set_variant(0)


@pytest.mark.parametrize("build", BUILDS)
def test_rows_host_rows_ranks_and_splits(renderer, build):
    check_rows_host_rows_ranks_and_splits(renderer, M.APP_OF[build], W, H, T, model_frame(build, W, H, T), cuts=[13, 14, 30], block_rows=8)


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
    # -DAPP_VINYL beside it, as a project that only adds the build's define would have: the build's define is tested first
    exe = build_dropin(tmp_path, ["APP_VINYL", "APP_VINYL_" + build.upper()], "APP_VINYL_" + build.upper())
    assert_same(run_dropin(exe, W, H, T, tmp_path), model_frame(build, W, H, T), ("dropin", build))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    assert_same(run_sbx_render(tmp_path, M.APP_OF[build], W, H, T), model_frame(build, W, H, T), ("sbx_render --app " + M.APP_OF[build],))


def test_shipped_builds_between_and_after_the_new_apps(renderer):
    """one context, the apps taking turns: SBX_APP_VINYL and SBX_APP_VINYL_GPU keep returning their own golden frames — no dispatch-order
    table and no cached frame crosses builds"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "vinyl_64x36.npz"))
    zg = np.load(os.path.join(ROOT, "tests", "golden", "vinyl_gpu_64x36.npz"))
    for key in ("t0.37", "t2.5"):
        t = float(key[1:])
        for build in BUILDS:
            assert_same(renderer.render(M.APP_OF[build], 64, 36, t), model_frame(build, 64, 36, t), (build, "in turn", t))
            assert_same(renderer.render("vinyl", 64, 36, t), z[key], ("vinyl after", build, t))
            assert_same(renderer.render("vinyl_gpu", 64, 36, t), zg[key], ("vinyl_gpu after", build, t))
    for build in BUILDS:
        assert_same(renderer.render(M.APP_OF[build], 64, 36, 2.5), model_frame(build, 64, 36, 2.5), (build, "at the end"))
    # the same at a shape that takes a table (32 x 132 tiles of 32 x 8 pixels; 64 x 36 is below the 4096 tiles one needs): runs long
    # enough for each app's table to be built and used, the apps taking turns twice — every frame is that app's first, a table IS there
    import torch
    w, h, t = 1000, 1051, 2.5
    first = {}
    for rnd in range(2):
        for app in [M.APP_OF[b] for b in BUILDS] + ["vinyl", "vinyl_gpu"]:
            for k in range(5):
                got = renderer.render(app, w, h, t)
                torch.cuda.synchronize()
                if app not in first:
                    first[app] = got.cpu().numpy()
                assert_same(got, first[app], (app, "round", rnd, "launch", k))
            assert renderer.tile_order(app)[0] >= 1, (app, rnd)
    for build in BUILDS:
        assert not M.same_bits(first[M.APP_OF[build]], first["vinyl"]).all(), build


def test_noshadow_equals_the_default_build_where_nothing_is_shadowed(renderer):
    """the model's `parts` of the shipped build: where sh is exactly 1, and on the background, NOSHADOW's pixel is SBX_APP_VINYL's"""
    for w, h, t in [(64, 36, 2.5), (97, 55, -3.7)]:
        parts = model("default", w, h, t)[1]
        unshadowed = (~parts["hit"] | (parts["sh"] == 1)).reshape(h, w)
        assert unshadowed.any() and (~unshadowed).any() and (~parts["hit"]).any()
        a = renderer.render("vinyl_noshadow", w, h, t).cpu().numpy()
        b = renderer.render("vinyl", w, h, t).cpu().numpy()
        assert_same(a[unshadowed], b[unshadowed], ("noshadow where sh == 1", w, h, t))
        assert not M.same_bits(a[~unshadowed], b[~unshadowed]).all()
