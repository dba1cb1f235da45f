"""Vectorised numpy restatement of SBX_APP_FUNC (src/app_func.h, its compiled `#if 1 // 2D` branch; include/sbx.h).

The reference does not compile as shipped (its ashima-noise submodule is absent), so it holds no answers for this shader: this module
IS the definition the GPU tests compare against, pinned by review and by tests/test_appfunc_cpu.py.  t and the combination are
binary32 in the written order (explicit np.float32 constants, so that nothing widens to float64); noise_w is the CPU oracle's
(Oracle.noise("noise_w"), pinned to SURVEY Appendix C by the existing parity tests).  This module also carries a pure-numpy binary32
hash_w / noise_w, which the CPU tests check against the oracle on every cell and grid position the frames reach.
"""
import concurrent.futures
import os

import numpy as np

from tests.model_common import F, ONE, mod, oracle, same_bits

HALF, W_OFF = F(.5), F(.015)
PERIODS = (4, 8, 16, 24, 32, 64)             # the distinct domain repeats of worley_tex_left / _middle / _right (:17-39)


def oracle_noise_w(xyz, L, chunk=1 << 16):
    """Oracle.noise("noise_w", xyz, (L, 0, 0)) -> float32 [n, 3], in chunks on a few threads (the ctypes call releases the GIL)"""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=F).reshape(-1, 3))
    o = oracle()
    parts = [xyz[i:i + chunk] for i in range(0, len(xyz), chunk)]
    if len(parts) <= 1:
        return o.noise("noise_w", xyz, (L, 0.0, 0.0))
    with concurrent.futures.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        return np.concatenate(list(ex.map(lambda p: o.noise("noise_w", p, (L, 0.0, 0.0)), parts)))


def t_of(width, height, fx, fy):
    """t = (fragCoord + .5) / u_res (:72), binary32; no y flip (that is the HLSL build only, :73-75)"""
    fx, fy = np.asarray(fx, dtype=F), np.asarray(fy, dtype=F)
    with np.errstate(all="ignore"):
        return (fx + HALF) / F(width), (fy + HALF) / F(height)


def combine(w):
    """worley_fbm (:41-47) over worley_tex_left / _middle / _right (:17-39) from w[L] = 1 - (noise_w(pos, L).r + .015), float32"""
    a, b, c = F(.625), F(.25), F(.125)
    with np.errstate(all="ignore"):
        left = w[4] * a + w[8] * b + w[16] * c
        middle = w[8] * a + w[16] * b + w[32] * c
        right = w[24] * a + w[32] * b + w[64] * c
        return (left * a + middle * b + right * c).astype(F)


def f1_of(tx, ty, noise=None):
    """{L: noise_w((tx, ty, 0), L).x} for the six periods (oracle noise_w unless another noise(xyz, L) is given)"""
    noise = noise or oracle_noise_w
    tx, ty = np.broadcast_arrays(np.asarray(tx, dtype=F), np.asarray(ty, dtype=F))
    xyz = np.stack([tx.ravel(), ty.ravel(), np.zeros(tx.size, dtype=F)], axis=-1)
    return {L: noise(xyz, L)[:, 0].reshape(tx.shape) for L in PERIODS}


def worley_fbm_xyz(xyz):
    """app_func.h's worley_fbm at arbitrary 3-D points (float32 [n])"""
    xyz = np.asarray(xyz, dtype=F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return combine({L: ONE - (oracle_noise_w(xyz, L)[:, 0] + W_OFF) for L in PERIODS})


def main_image(width, height, fx, fy):
    """fragColor = (n, n, n, 1) at fragCoords (fx, fy) -> float32 [..., 4]"""
    tx, ty = t_of(width, height, fx, fy)
    f1 = f1_of(tx, ty)
    with np.errstate(all="ignore"):
        n = combine({L: ONE - (f1[L] + W_OFF) for L in PERIODS})
    return np.stack([n, n, n, np.ones_like(n)], axis=-1).astype(F)


def frame(width, height, rows=None):
    """float32 [rows, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre).  u_time and u_mouse do not enter."""
    ys = np.arange(height) if rows is None else np.asarray(list(rows))
    fx = (np.arange(width, dtype=F) + HALF)[None, :]
    fy = (ys.astype(F) + HALF)[:, None]
    fx, fy = np.broadcast_arrays(fx, fy)
    return main_image(width, height, fx, fy)


# ---- pure numpy binary32 hash_w / noise_w (src/noise_worley.h:5-51) -------------------------------------------------------------
def _dot(a, b):                              # ((a0 b0 + a1 b1) + a2 b2), binary32
    return (a[..., 0] * F(b[0]) + a[..., 1] * F(b[1])) + a[..., 2] * F(b[2])


def _sin(x):                                 # the correctly rounded binary32 sin of the math spec, through binary64
    return np.sin(np.asarray(x, dtype=F).astype(np.float64)).astype(F)


def _fract(x):
    return x - np.floor(x)


def hash_w(x):
    """hash_w over points float32 [..., 3] -> float32 [..., 3]"""
    x = np.asarray(x, dtype=F)
    k = F(43758.5453123)
    with np.errstate(all="ignore"):
        xx = [_dot(x, (127.1, 311.7, 74.7)), _dot(x, (269.5, 183.3, 246.1)), _dot(x, (113.5, 271.9, 124.6))]
        return np.stack([_fract(_sin(v) * k) for v in xx], axis=-1).astype(F)


def noise_w_numpy(xyz, L):
    """noise_w(pos, L) over points float32 [n, 3] -> [n, 3] with only .x (sqrt F1) filled: F2 and the cell id are unused here"""
    pos = np.asarray(xyz, dtype=F).reshape(-1, 3)
    rep = F(L)
    with np.errstate(all="ignore"):
        x = pos * rep
        p = np.floor(x)
        f = x - p
        r0 = np.full(len(pos), F(100), dtype=F)
        for k in (-1, 0, 1):
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    b = np.array([i, j, k], dtype=F)
                    pb = p + b
                    r = (b - f) + hash_w(mod(pb, rep))
                    d = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]          # dot(r, r)
                    r0 = np.where(d < r0, d, r0)
        out = np.zeros_like(pos)
        out[:, 0] = np.sqrt(r0)
    return out


def table_cells():
    """every hash_w argument APP_FUNC's frames can reach from pos.z = 0: (x, y, mod(z, L)) for L in PERIODS, x, y in [0, L),
    z in -1, 0, 1, in the table order of kern_func.hip -> float32 [18096, 3]"""
    cells = []
    for L in PERIODS:
        fL = F(L)
        for kz in range(3):
            z = mod(F(kz - 1), fL)
            y, x = np.meshgrid(np.arange(L, dtype=F), np.arange(L, dtype=F), indexing="ij")
            cells.append(np.stack([x.ravel(), y.ravel(), np.full(L * L, z, dtype=F)], axis=-1))
    return np.concatenate(cells).astype(F)
