"""CPU tests of the SBX_APP_ATMOSPHERE_GROUND model (tests/atmosphere_ground_model.py) and of the host-only layers of the app:
the numpy vector algebra against the oracle's compiled code, the facts include/sbx.h states about the frame, the Python app
table and sbx_span_table (which needs the built library but no GPU)."""
import numpy as np
import pytest

from tests import atmosphere_ground_model as M

F = np.float32


def test_primary_ray_equals_the_oracle_hook(oracle):
    """get_primary_ray of the model == the oracle's `primary_ray` hook, bit for bit, for three cameras over a grid of point_cam"""
    from oracle.oracle import APP_ATMOSPHERE, APP_CLOUDS, APP_EGG
    cams = {APP_EGG: ((0, .25, 5.25), (0, .25, 0)),              # oracle/ref_apps.h setup_camera of each app (u_mouse = 0)
            APP_CLOUDS: ((0, -.5, 0), (0, 0, -1)),
            APP_ATMOSPHERE: ((0, 0, 0), (0, 1, 0))}
    xs = np.concatenate([np.linspace(-1.9, 1.9, 23), [0, 1e-8, -1e6, 3e19, np.inf, np.nan]]).astype(F)
    ys = np.concatenate([np.linspace(-1.1, 1.1, 19), [0, -0.5590170, 1e7, -3e19, -np.inf, np.nan]]).astype(F)
    gx, gy = [a.ravel() for a in np.meshgrid(xs, ys)]
    for app, (eye, look_at) in cams.items():
        got = np.stack(M.get_primary_ray(gx, gy, eye, look_at), axis=-1)
        for i in range(len(gx)):
            want = oracle.kat("primary_ray", [app, 96, 54, 0, 0, .37, gx[i], gy[i], -1], 6)
            assert M.same_bits(got[i], want[:3]).all(), (app, gx[i], gy[i], got[i], want[:3])
            assert M.same_bits(np.array(eye, dtype=F), want[3:]).all()


def test_point_cam_and_camera_constants():
    """the y values of the ground camera are exact in binary32; point_cam stays binary32 and follows main.h:40,44-46"""
    assert float(M.EYE[1]) == 6360001.0 and float(M.LOOK_AT[1]) == 6360001.5
    pcx, pcy = M.point_cam(96, 54, np.arange(96, dtype=F) + F(.5), F(13.5))
    assert pcx.dtype == F and pcy.dtype == F
    assert float(pcx[0]) == float((F(2) * (F(.5) / F(96)) - F(1)) * (F(96) / F(54)))


def test_sun_equals_the_oracle_hook(oracle):
    for t in (0, .37, 2, 3.1, 100.25):
        assert M.same_bits(M.sun_dir(t), oracle.kat("atmosphere.sun_dir", [96, 54, 0, 0, t], 3)).all()
        assert abs(float(np.linalg.norm(M.sun_dir(t).astype(np.float64))) - 1) < 1e-6


def test_frame_facts(oracle):
    w, h = 96, 54
    assert M.horizon_row(w, h) == 12
    grey = oracle.math("pow", np.array([.33], dtype=F), F(1) / F(2.2))[0]
    for t in (.37, 2.0, 3.1):
        f = M.frame(w, h, t)
        assert f.shape == (h, w, 4) and f.dtype == F
        assert np.isfinite(f).all()
        assert (f[..., 3] == 1).all()
        assert (f[:12, :, :3] == grey).all()                      # rows 0-11: ground, whole rows (no roll)
        assert (f[12:, :, :3] != grey).any(axis=-1).all()         # every pixel above: sky
    assert M.frame(w, h, 2.0)[..., :3].max() > 1.5                # sky channels exceed 1 near the sun, unclamped


def test_nan_direction_is_ground(oracle):
    grey = oracle.math("pow", np.array([.33], dtype=F), F(1) / F(2.2))[0]
    pts = np.array([[np.nan, 5], [5, np.nan], [np.nan, np.nan]], dtype=F)
    got = M.main_image(1920, 1080, .37, pts[:, 0], pts[:, 1])
    assert (got[:, :3] == grey).all() and (got[:, 3] == 1).all()
    # straight up and a hair either side of denom = 1e-6 go where the comparison sends them
    t = M.intersect_plane_t((np.array([0, 0, 0], dtype=F), np.array([1, -9e-7, -1.1e-6], dtype=F), np.array([0, 1, 1], dtype=F)))
    assert t[0] == M.NO_HIT_T and t[1] == M.NO_HIT_T and t[2] < M.MAX_DIST


def test_app_id_and_names():
    import shaderbox_amd
    assert shaderbox_amd.app_id("atmosphere_ground") == 16
    assert shaderbox_amd.app_id("APP_ATMOSPHERE_GROUND") == 16
    assert shaderbox_amd.app_id("atmosphere") == 5


@pytest.mark.parametrize("w,h,br", [(1920, 1080, 8), (7680, 4320, 16), (96, 54, 4)])
def test_span_table_moves_only_sky(w, h, br):
    """sbx_span_table (host only): blocks wholly under the horizon carry no span, sky blocks span their whole width"""
    import shaderbox_amd
    hz = M.horizon_row(w, h)
    table, pix, maxw = shaderbox_amd.span_table("atmosphere_ground", w, h, .37, br, 4)
    assert table.shape == ((h + br - 1) // br, 4)
    for g, (x0, x1, off, owner) in enumerate(table):
        ya, yb = g * br, min(h, (g + 1) * br) - 1
        if yb < hz:
            assert x0 == x1, ("a block under the horizon has a span", g, x0, x1)
        else:
            assert (x0, x1) == (0, w), ("a block with sky rows must span its width", g, x0, x1)
    assert maxw == w
    rows = np.minimum(h, (np.arange(len(table)) + 1) * br) - np.arange(len(table)) * br
    assert int(pix.sum()) == int((rows * (table[:, 1] - table[:, 0])).sum())
    assert int(pix.sum()) < w * h
