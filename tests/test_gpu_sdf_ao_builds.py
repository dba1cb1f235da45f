"""GPU tests of SBX_APP_SDF_AO_SHADOW and SBX_APP_SDF_AO_NORMALS (src/app_sdf_ao.h with one of its `#if 0` blocks on; include/sbx.h,
DESIGN.md §5.11): every layer bit for bit, NaN == NaN, all four channels, against tests/sdf_ao_builds_model.py — and, at 64x36,
against the frames the edited reference header rendered (tests/golden/sdf_ao_builds/)."""
import numpy as np
import pytest

from tests import sdf_ao_builds_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, edge_points, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

BUILDS = ["shadow", "normals"]
F = np.float32


_frame = frame_cache(M.frame)


def model_frame(build, w, h, t, aux=None):
    return _frame(build, w, h, t, aux)


def aux_block(aux):
    import shaderbox_amd
    if aux is None:
        return None
    a = shaderbox_amd.AuxSdfAo()
    a.fog_density, a.fog_falloff = aux
    return a


def golden(build):
    z = M.fixture(build)
    return [(float(u[4]), f) for u, f in zip(z["uniforms"], z["frames"])]


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


@pytest.mark.parametrize("build", BUILDS)
def test_points_and_main_image(renderer, build):
    import torch
    app = "sdf_ao_" + build
    w, h = 1920, 1080
    pts = edge_points(w, h)
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
    pts = torch.from_numpy(edge_points(w, h))
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
    w, h, br, t = 640, 360, 8, 2.5
    aux = (0.02, 1.5)
    check_rows_host_rows_ranks_and_splits(renderer, "sdf_ao_" + build, w, h, t, model_frame(build, w, h, t, aux), cuts=[13, 14, 300],
                                          block_rows=br, aux=aux_block(aux))


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, build, n):
    """the span exchange (whole rows: no cost model, as APP_SDF_AO) and the direct exchange's rgb slabs, every rank's schedule on this GPU"""
    w, h, t = 1000, 333, 2.5
    check_loopback_exchanges(renderer, "sdf_ao_" + build, n, w, h, t)


@pytest.mark.parametrize("build", BUILDS)
def test_rgba8_frames(renderer, build):
    w, h, t = 800, 450, 2.5
    check_rgba8(renderer, "sdf_ao_" + build, w, h, t)


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
    w, h, t = 1280, 720, 2.5
    check_multi_render("sdf_ao_" + build, w, h, t, lambda: model_frame(build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_cpp_dropin(tmp_path, build):
    # -DAPP_SDF_AO beside it, as a project that only adds the build's define would have: the build's define is tested first
    exe = build_dropin(tmp_path, ["APP_SDF_AO", "APP_SDF_AO_" + build.upper()], "APP_SDF_AO_" + build.upper())
    for w, h, t in [(320, 180, 0.37), (97, 61, 9.25)]:
        assert_same(run_dropin(exe, w, h, t, tmp_path), model_frame(build, w, h, t), ("dropin", build, w, h, t))


@pytest.mark.parametrize("build", BUILDS)
def test_sbx_render_host(tmp_path, build):
    w, h = 257, 130
    for t, aux, flags in [(0.37, None, []), (2.5, (0.25, 1.5), ["--fog-density", "0.25", "--fog-falloff", "1.5"])]:
        got = run_sbx_render(tmp_path, "sdf_ao_" + build, w, h, t, flags)
        assert_same(got, model_frame(build, w, h, t, aux), ("sbx_render --app sdf_ao_" + build, t, aux))
