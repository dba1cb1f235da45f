"""Vectorised numpy restatement of SBX_APP_2D / SBX_APP_2D_TEX (src/app_2d.h:70-111; include/sbx.h).

The CPU oracle does not implement this shader: the GPU tests compare against this module, and this module is compared bit for
bit with src/app_2d.h itself, compiled verbatim in both of its forms (oracle/_ref/libsbx_ref_2d.so and _2d_tex.so;
tests/test_oracle_vs_reference.py), besides tests/test_app2d_cpu.py.  Every step is binary32 in the written order (explicit
np.float32 constants, so that nothing widens to float64); atan is the binary64 atan2 of the math spec, taken from the oracle
(oracle.math("atan2"), which only reads oracle/).  Divisions are the plain IEEE binary32 quotients — the kernel's multiplies by a
binary64 reciprocal (div_by, sbx_math.h) are proven equal to them, and the GPU tests check that they are.
"""
import numpy as np

from tests.model_common import F, ONE, TWO, ZERO, fmax, mod, oracle, same_bits

PI = F(3.14159265359)                       # src/def.h:51
HALF, FOUR, TWELVE, SIXTEEN = F(.5), F(4), F(12), F(16)


def _atan2(y, x):
    y = np.ascontiguousarray(y, dtype=F)
    x = np.ascontiguousarray(np.broadcast_to(x, y.shape), dtype=F)
    return oracle().math("atan2", y.ravel(), x.ravel()).reshape(y.shape)


def phase(u_time):
    """(phase, time, w) that the host decides once per frame: t = mod(u_time, 16) and the strict inequalities of :82-103;
    phase 4 = none of the branches runs (t = 4, 8, 12 or NaN)."""
    ut = F(u_time)
    with np.errstate(all="ignore"):
        t = mod(ut, SIXTEEN)
        if t < FOUR:
            return 0, ut, ZERO
        if t > FOUR and t < F(8):
            return 1, ONE, (t - FOUR) / FOUR
        if t > F(8) and t < TWELVE:
            return 2, ut, ZERO
        if t > TWELVE:
            return 3, ONE, (t - TWELVE) / FOUR
    return 4, ONE, ZERO


def perturb_tunnel(ux, uy, time):           # :49-62, returns (s, t, r)
    px, py = TWO * ux - ONE, TWO * uy - ONE
    r = np.sqrt(px * px + py * py)
    a = _atan2(py, px) + time
    return ONE / r + time, FOUR * (a / PI), r


def perturb_road(ux, uy, time):             # :37-47
    px, py = TWO * ux - ONE, TWO * uy - ONE
    ay = np.abs(py)
    return px / ay, ONE / ay - time


def checkerboard(x, y):                     # checkboard_pattern(uv, 2.), src/util.h:95-101, as vec4(cb, cb, cb, 1)
    cb = mod(np.floor(x * TWO) + np.floor(y * TWO), TWO)
    return np.stack([cb, cb, cb, np.ones_like(cb)], axis=-1)


def _tex_axis(c, size):                     # the spec's WRAP (kern_2d.hip tex2_axis)
    fs = F(size)
    u = c * fs - HALF
    fl = np.floor(u)
    f = u - fl
    m = fl - fs * np.floor(fl / fs)
    m = np.where(m < ZERO, m + fs, m)
    m = np.where(m >= fs, m - fs, m)
    ok = (m >= ZERO) & (m < fs)
    i0 = np.where(ok, m, ZERO).astype(np.int64)
    i1 = np.where(i0 + 1 == size, 0, i0 + 1)
    return i0, i1, f.astype(F)


def _mix(a, b, w):                          # GLSL mix: a (1 - w) + b w
    return a * (ONE - w) + b * w


def texture(tex, x, y):
    """bilinear WRAP sample of tex (float32 [h, w, 4], row 0 at v = 0): mix in x, then in y"""
    h, w = tex.shape[:2]
    x0, x1, fx = _tex_axis(x, w)
    y0, y1, fy = _tex_axis(y, h)
    fx, fy = fx[..., None], fy[..., None]
    return _mix(_mix(tex[y0, x0], tex[y0, x1], fx), _mix(tex[y1, x0], tex[y1, x1], fx), fy).astype(F)


def decode_unorm8(words):
    """R8G8B8A8_UNORM words [h, w] -> float32 [h, w, 4], c / 255 correctly rounded (binary32 division)"""
    w = np.asarray(words, dtype=np.uint32)
    return np.stack([((w >> s) & 255).astype(F) / F(255) for s in (0, 8, 16, 24)], axis=-1).astype(F)


def checkerboard_texture(size=128, freq=16):  # hlsltoy's CreateTextureCheckboard (util/hlsltoy/src/hlsltoy.cpp:66-87)
    i = np.arange(size, dtype=np.uint32)
    same = (i[None, :] & np.uint32(freq)) == (i[:, None] & np.uint32(freq))
    return np.where(same, np.uint32(0xff000000), np.uint32(0xffffffff)).astype(np.uint32)


def intermediates(width, height, u_time, fx, fy):
    """(st, d, g) of mainImage at fragCoords (fx, fy): the sample coordinate, the tunnel's r (1 in the road phase) and the
    factor 1 - tent_filter(2 uv.y - 1).  st is None in the undefined phase."""
    fx, fy = np.asarray(fx, dtype=F), np.asarray(fy, dtype=F)
    with np.errstate(all="ignore"):
        ux, uy = fx / F(width), fy / F(height)                  # :72
        ph, time, w = phase(u_time)
        d = np.ones_like(ux)
        st = None
        if ph == 0:
            s, t, d = perturb_tunnel(ux, uy, time)
            st = (s, t)
        elif ph in (1, 3):
            s, t, d = perturb_tunnel(ux, uy, time)
            s2, t2 = perturb_road(ux, uy, time)
            a, b = ((s, t), (s2, t2)) if ph == 1 else ((s2, t2), (s, t))
            st = (_mix(a[0], b[0], w), _mix(a[1], b[1], w))
        elif ph == 2:
            st = perturb_road(ux, uy, time)
        g = ONE - fmax(ONE - np.abs(TWO * uy - ONE), ZERO)     # :64-68, 106
    return st, d, g


def main_image(width, height, u_time, fx, fy, tex=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]; tex = None: the checkerboard sample() of APP_2D, else the float32
    texels of APP_2D_TEX's t0"""
    st, d, g = intermediates(width, height, u_time, fx, fy)
    ph = phase(u_time)[0]
    with np.errstate(all="ignore"):
        if st is None:
            color = np.zeros(np.shape(g) + (4,), dtype=F)
        else:
            color = checkerboard(*st) if tex is None else texture(tex, *st)
            if ph != 2:
                color = color * d[..., None]
        return (color * g[..., None]).astype(F)


def frame(width, height, u_time, tex=None, rows=None):
    """float32 [rows, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre)"""
    ys = np.arange(height) if rows is None else np.asarray(list(rows))
    fx = (np.arange(width, dtype=F) + HALF)[None, :]
    fy = (ys.astype(F) + HALF)[:, None]
    fx, fy = np.broadcast_arrays(fx, fy)
    return main_image(width, height, u_time, fx, fy, tex)
