"""GPU tests of SBX_APP_FUNC (src/app_func.h's 2D branch; include/sbx.h): every layer bit for bit, NaN == NaN, all four channels,
against the restatement of tests/appfunc_model.py (oracle noise_w, binary32 combination)."""
import numpy as np
import pytest

from tests import appfunc_model as M
from tests.app_checks import (assert_same, build_dropin, check_loopback_exchanges, check_multi_render, check_rgba8,
                              check_rows_host_rows_ranks_and_splits, edge_points, frame_cache, run_dropin, run_sbx_render)
from tests.app_checks import renderer  # noqa: F401 (the module-scoped fixture)

pytestmark = pytest.mark.gpu

model_frame = frame_cache(M.frame)


@pytest.mark.parametrize("w,h", [(1, 1), (7, 3), (33, 9), (257, 2), (640, 360), (1920, 1080)])
def test_frames(renderer, w, h):
    want = model_frame(w, h)
    assert (want[..., 3] == 1).all()
    for t, mouse in [(0.37, (0.0, 0.0)), (123.25, (50.0, 60.0)), (-7.0, (-3.0, 1e6))]:    # u_time and u_mouse do not enter
        assert_same(renderer.render("func", w, h, t, mouse=mouse), want, (w, h, t, mouse))


def test_points_and_main_image(renderer):
    import torch
    w, h = 1920, 1080
    pts = edge_points(w, h)
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
    pts = torch.from_numpy(edge_points(w, h))
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
    w, h, br = 640, 360, 8
    check_rows_host_rows_ranks_and_splits(renderer, "func", w, h, 0.37, model_frame(w, h), cuts=[13, 14, 300], block_rows=br)


@pytest.mark.parametrize("n", [2, 3])
def test_exchanges_through_loopback_ranks(renderer, n):
    """the span exchange (whole rows: no cost model) and the direct exchange's rgb slabs, every rank's schedule on this GPU"""
    w, h = 1000, 333
    check_loopback_exchanges(renderer, "func", n, w, h, 0.37)


def test_rgba8_frames(renderer):
    w, h = 800, 450
    check_rgba8(renderer, "func", w, h, 0.37)


def test_multi_render(renderer):
    w, h = 1280, 720
    check_multi_render("func", w, h, 0.37, lambda: model_frame(w, h))


def test_cpp_dropin(tmp_path):
    exe = build_dropin(tmp_path, ["APP_FUNC"], "APP_FUNC")
    for w, h, t in [(320, 180, 0.37), (97, 61, 9.25)]:
        assert_same(run_dropin(exe, w, h, t, tmp_path), model_frame(w, h), ("dropin", w, h, t))


def test_sbx_render_host(tmp_path):
    w, h = 257, 130
    assert_same(run_sbx_render(tmp_path, "func", w, h, 0.37), model_frame(w, h), "sbx_render --app func")
