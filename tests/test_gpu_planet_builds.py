"""GPU tests of SBX_APP_PLANET_CLOSEUP, SBX_APP_PLANET_CLOUDLESS and SBX_APP_PLANET_UNLIT (src/app_planet.h with its `#if 0` at :51 on
/ without its `#define CLOUDS` at :63 / without its `#define LIGHT` at :249; include/sbx.h): every layer bit for
bit, NaN == NaN, all four channels, against the frames and points the edited reference header rendered
(tests/golden/planet_builds/) and against tests/planet_builds_model.py."""
import os

import numpy as np
import pytest

from tests import planet_builds_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)
from tests.model_common import same_bits

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = ["closeup", "cloudless", "unlit"]
W, H, T = 64, 36, 2.5                                                   # the layer checks' frame


def _model(build, w, h, t):
    parts = {}
    return (M.frame(build, w, h, t, parts=parts), parts)


model = frame_cache(_model)


def model_frame(build, w, h, t):
    return model(build, w, h, t)[0]


@pytest.mark.parametrize("build", BUILDS)
def test_reference_frames_and_points(renderer, build):
    """what src/app_planet.h itself rendered with the one line edited, from the default kernel and the plain one"""
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
def test_frame_whose_size_is_no_multiple_of_the_tile(renderer, build):
    w, h = 97, 55                                                       # 8-wide, 8-row wave tiles
    for t in (2.5, -3.7):
        assert_same(renderer.render(M.APP_OF[build], w, h, t), model_frame(build, w, h, t), (build, w, h, t))


def _times():
    """six seeded u_time; inf and NaN, which tame_time sends to the plain kernels whatever the variant; 2e8, beyond tame_time"""
    rng = np.random.default_rng(37)
    return [float(t) for t in rng.uniform(-20, 20, size=6)] + [float("inf"), float("nan"), 2e8]


@pytest.mark.parametrize("build", BUILDS)
def test_default_and_plain_kernels_agree(renderer, build):
    w, h = 256, 144
    app = M.APP_OF[build]
    try:
        for t in _times():
            got = {}
            for v in (0, 1):
                renderer.set_variant(v)
                got[v] = renderer.render(app, w, h, t).cpu().numpy()
            assert_same(got[1], got[0], (build, t, "variant 0 vs 1"))
            assert (got[0][..., 3] == 1).all()
            renderer.set_variant(0)
            if np.isfinite(t):
                shipped = renderer.render("planet", w, h, t).cpu().numpy()
                assert not same_bits(got[0], shipped).all(), (build, t, "the shipped build's frame")
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
    # -DAPP_PLANET beside it, as a project that only adds the build's define would have: the build's define is tested first
    exe = build_dropin(tmp_path, ["APP_PLANET", "APP_PLANET_" + build.upper()], "APP_PLANET_" + build.upper())
    assert_same(run_dropin(exe, W, H, T, tmp_path), model_frame(build, W, H, T), ("dropin", build))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    assert_same(run_sbx_render(tmp_path, M.APP_OF[build], W, H, T), model_frame(build, W, H, T), ("sbx_render --app " + M.APP_OF[build],))


def test_shipped_builds_between_and_after_the_new_apps(renderer):
    """one context, the apps taking turns: SBX_APP_PLANET and SBX_APP_PLANET_ATMOSPHERE keep returning their own golden frames"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "planet_64x36.npz"))
    za = np.load(os.path.join(ROOT, "tests", "golden", "planet_atmosphere_64x36.npz"))
    for key in ("t0.37", "t2.5"):
        t = float(key[1:])
        for build in BUILDS:
            assert_same(renderer.render(M.APP_OF[build], 64, 36, t), model_frame(build, 64, 36, t), (build, "in turn", t))
            assert_same(renderer.render("planet", 64, 36, t), z[key], ("planet after", build, t))
            assert_same(renderer.render("planet_atmosphere", 64, 36, t), za[key], ("planet_atmosphere after", build, t))
    for build in BUILDS:
        assert_same(renderer.render(M.APP_OF[build], 64, 36, 2.5), model_frame(build, 64, 36, 2.5), (build, "at the end"))


def test_unlit_equals_the_default_build_off_the_ground(renderer):
    """the model's `parts` of the shipped build: without a ground hit illuminate does not run, and UNLIT's pixel is SBX_APP_PLANET's"""
    for w, h, t in [(64, 36, 2.5), (97, 55, -3.7)]:
        parts = model("default", w, h, t)[1]
        sky = (~parts["ground"]).reshape(h, w)
        assert sky.any() and (~sky).any() and (~parts["atm"]).any()
        a = renderer.render("planet_unlit", w, h, t).cpu().numpy()
        b = renderer.render("planet", w, h, t).cpu().numpy()
        assert_same(a[sky], b[sky], ("unlit off the ground", w, h, t))
        assert not same_bits(a[~sky], b[~sky]).all()


def test_cloudless_equals_the_default_build_where_no_cloud_enters(renderer):
    """the model's `parts` of the shipped build: where the view march leaves alpha exactly 0 and the shadow is exactly 1"""
    for w, h, t in [(64, 36, 2.5), (97, 55, -3.7)]:
        parts = model("default", w, h, t)[1]
        clear = ((parts["alpha"] == 0) & (parts["shadow"] == 1)).reshape(h, w)
        assert clear.any() and (~clear).any() and (clear & parts["ground"].reshape(h, w)).any()
        a = renderer.render("planet_cloudless", w, h, t).cpu().numpy()
        b = renderer.render("planet", w, h, t).cpu().numpy()
        assert_same(a[clear], b[clear], ("cloudless where no cloud enters", w, h, t))
        assert not same_bits(a[~clear], b[~clear]).all()
