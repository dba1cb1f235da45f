"""CPU tests of SBX_APP_2D / SBX_APP_2D_TEX (src/app_2d.h): the numpy restatement (tests/app2d_model.py) against a float64
evaluation of the same formulas, the checkerboard texture against hlsltoy's rule, the Python surface and the header."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import app2d_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"


def _f64(width, height, u_time, fx, fy):
    """the same mainImage intermediates in float64 (atan2 from numpy), phase and weight from the binary32 host decision"""
    ph, time, w = M.phase(u_time)
    ux, uy = fx.astype(np.float64) / width, fy.astype(np.float64) / height
    px, py = 2 * ux - 1, 2 * uy - 1
    r = np.sqrt(px * px + py * py)
    tun = (1 / r + float(time), 4 * ((np.arctan2(py, px) + float(time)) / float(M.PI)))
    road = (px / np.abs(py), 1 / np.abs(py) - float(time))
    w = float(w)
    d = np.ones_like(ux)
    if ph == 0:
        st, d = tun, r
    elif ph == 1:
        st, d = ((tun[0] * (1 - w) + road[0] * w), (tun[1] * (1 - w) + road[1] * w)), r
    elif ph == 2:
        st = road
    else:
        st, d = ((road[0] * (1 - w) + tun[0] * w), (road[1] * (1 - w) + tun[1] * w)), r
    g = 1 - np.maximum(1 - np.abs(2 * uy - 1), 0)
    # the magnitude a component is computed from: the time added or subtracted, and in the mixed phases both coordinates (a
    # tunnel and a road coordinate of opposite signs, or 1 / |p.y| and the time, cancel)
    scale = tuple(np.maximum(np.maximum(np.abs(a), np.abs(b)), 2 * abs(float(time))) for a, b in zip(tun, road))
    return st, d, d * g, scale


@pytest.mark.parametrize("u_time", [0.37, 2.0, 5.5, 9.25, 13.0, 14.0, -3.1, 1000.9])
def test_restatement_matches_float64(u_time):
    W, H = 1920, 1080
    fx, fy = np.meshgrid(np.arange(0, W, 7, dtype=np.float32) + .5, np.arange(0, H, 5, dtype=np.float32) + .5)
    st, d, g = M.intermediates(W, H, u_time, fx, fy)
    st64, d64, alpha64, scale = _f64(W, H, u_time, fx, fy)
    ph = M.phase(u_time)[0]
    alpha = (d * g) if ph != 2 else g
    # away from r = 0 (the tunnel's 1 / r) and from |p.y| = 0 (the road's 1 / |p.y|), where a rounding of uv is amplified without bound
    p = np.hypot(2 * fx / W - 1, 2 * fy / H - 1)
    py = np.abs(2 * fy.astype(np.float64) / H - 1)
    keep = (p > .05) & (py > .05)
    for got, want, sc in [(st[0], st64[0], scale[0]), (st[1], st64[1], scale[1]), (d, d64, d64), (alpha, alpha64, alpha64)]:
        got, want, sc = got[keep].astype(np.float64), want[keep], sc[keep]
        rel = np.abs(got - want) / np.maximum(np.maximum(np.abs(want), sc), 1.0)
        assert rel.max() < 1e-6, (u_time, float(rel.max()))
    # and the phase decision itself, the reference's strict inequalities (app_2d.h:82-103)
    assert M.phase(2.0)[0] == 0 and M.phase(6.0)[0] == 1 and M.phase(10.0)[0] == 2 and M.phase(14.0)[0] == 3
    assert [M.phase(t)[0] for t in (4.0, 8.0, 12.0, 16.0 + 4.0, float("nan"), float("inf"))] == [4] * 6


def test_undefined_phase_is_zero_times_tent():
    c = M.frame(64, 36, 8.0)
    assert c.shape == (36, 64, 4) and not c.any()
    assert not M.frame(16, 8, 12.0).any()


def test_texture_wrap_reads_inside():
    tex = np.arange(5 * 3 * 4, dtype=np.float32).reshape(3, 5, 4)
    c = np.array([0.0, .1, -.3, 1e9, -1e9, 3e38, np.inf, -np.inf, np.nan, 2.0 ** 31, -2.0 ** 33], dtype=np.float32)
    for size in (1, 3, 5, 97, 16384):
        i0, i1, f = M._tex_axis(c, size)
        assert ((i0 >= 0) & (i0 < size) & (i1 >= 0) & (i1 < size)).all()
    out = M.texture(tex, c, c[::-1])
    assert out.shape == (len(c), 4)
    # texel centres sample exactly: (i + .5) / w, (j + .5) / h
    x = (np.arange(5, dtype=np.float32) + .5) / np.float32(5)
    y = np.full(5, (1 + .5) / 3, dtype=np.float32)
    assert (M.texture(tex, x, y) == tex[1]).all()


def test_checkerboard_texture_matches_hlsltoy_rule():
    import shaderbox_amd
    py = shaderbox_amd.checkerboard_texture()
    assert py.shape == (128, 128) and py.dtype == np.uint32
    for y in range(128):
        for x in range(0, 128, 3):
            assert py[y, x] == (0xff000000 if (x & 16) == (y & 16) else 0xffffffff)
    assert (M.checkerboard_texture() == py).all()
    assert (shaderbox_amd.checkerboard_texture(40, 4) == M.checkerboard_texture(40, 4)).all()
    lib = shaderbox_amd.load_library()
    for size, freq in [(128, 16), (37, 8), (1, 16)]:
        out = np.zeros((size, size), dtype=np.uint32)
        lib.sbx_checkerboard_texture(size, freq, ctypes.c_void_p(out.ctypes.data))
        assert (out == shaderbox_amd.checkerboard_texture(size, freq)).all(), (size, freq)
    dec = M.decode_unorm8(py)
    assert set(np.unique(dec)) == {0.0, 1.0} and (dec[..., 3] == 1).all()


def test_python_accepts_app_names():
    import shaderbox_amd
    assert shaderbox_amd.app_id("2d") == shaderbox_amd.APP_2D == 13
    assert shaderbox_amd.app_id("2d_tex") == shaderbox_amd.APP_2D_TEX == 14
    assert shaderbox_amd.app_id("APP_2D") == 13 and shaderbox_amd.app_id("app_2d_tex") == 14
    assert shaderbox_amd.Renderer.set_texture2d


def test_header_declares_app2d():
    h = open(os.path.join(ROOT, "include", "sbx.h")).read()
    assert re.search(r"SBX_APP_2D\s*=\s*13\s*,", h) and re.search(r"SBX_APP_2D_TEX\s*=\s*14\b", h)
    assert re.search(r"int\s+sbx_set_texture2d\(sbx_ctx\*\s*ctx,\s*int\s+width,\s*int\s+height,\s*int\s+format,\s*const\s+void\*\s*texels,"
                     r"\s*void\*\s*stream\);", h)
    assert re.search(r"void\s+sbx_checkerboard_texture\(int\s+size,\s*int\s+freq,\s*uint32_t\*\s*out\);", h)
    assert "#define SBX_ABI_VERSION 2" in h
    hpp = open(os.path.join(ROOT, "include", "sbx_mainimage.hpp")).read()
    assert "defined(APP_2D)" in hpp and "defined(APP_2D_TEX)" in hpp
    lib = open(os.path.join(ROOT, "shaderbox_amd", "lib", "libsbx.so"), "rb").read()
    assert b"sbx_set_texture2d" in lib and b"sbx_checkerboard_texture" in lib


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference tree is not on this machine")
def test_reference_constants_app2d():
    src = open(os.path.join(REF, "src", "app_2d.h")).read()
    for text in ["float t = mod (u_time, 16.);", "if (t < 4.) {", "if (t > 4. && t < 8.) {", "(t - 4.) / 4.", "if (t > 8. && t < 12.) {",
                 "if (t > 12.) {", "(t - 12.) / 4.", "float t = 4. * (a / PI);", "checkboard_pattern(uv, 2.)",
                 "color *= 1. - tent_filter (2.*uv.y - 1.);", "return max (1. - abs (t) , 0);"]:
        assert text in src, text
    assert "#define PI 3.14159265359" in open(os.path.join(REF, "src", "def.h")).read()
    assert M.PI == np.float32(3.14159265359)
    host = open(os.path.join(REF, "util", "hlsltoy", "src", "hlsltoy.cpp")).read()
    assert "CreateTextureCheckboard(pd3dDevice, 128, 128, 16)" in host
    assert "((x & checkFreq) == (y & checkFreq)) ? 0xff000000 : 0xffffffff" in host
