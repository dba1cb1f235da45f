"""The three builds of src/app_clouds.h's illuminate_volume (:91-123), which holds two `#if 0` switches, restated in numpy binary32
step by step in the oracle's operation order (oracle/ref_apps.h AppClouds, oracle/ref_lib.h, oracle/ovec.h):
    "default"     the file as shipped                                           SBX_APP_CLOUDS
    "height"      the `#if 0` of :97 on: luminance = exp(height) / 2., no light march        SBX_APP_CLOUDS_HEIGHT
    "luminance"   the `#if 0` of :118 on: illuminate_volume returns its transmittance       SBX_APP_CLOUDS_LUMINANCE
The procedural build only (SKY_SPHERE and USE_NOISE_TEX undefined).  noise_iq is the oracle's (Oracle.noise), exp and pow are the
math spec's (Oracle.math); everything else is np.float32 arithmetic, one rounding per operation.  Vectorised over the pixels: the
march parameter t is the same for every pixel, so a step is one batch of density_func over the pixels still marching.

The definition is pinned from two sides (tests/test_clouds_builds_cpu.py): "default" equals the oracle in every bit, "height" and
"luminance" equal the frames and points that the edited reference header itself rendered (tests/golden/clouds_builds/,
tools/make_golden_builds.py)."""
import functools

import numpy as np

from oracle import aux_sets
from tests.model_common import F, ONE, TWO, ZERO, _f, builds_fixture, dot, fmax, fmin, get_primary_ray, oracle, point_cam, same_bits  # noqa: F401

BUILDS = ("default", "height", "luminance")
APP_OF = {"default": "clouds", "height": "clouds_height", "luminance": "clouds_luminance"}
FOV = F(1.)                                         # app_clouds.h:220
HG_G = F(.2)                                        # :5
PI = F(3.14159265359)                               # def.h:51
NOISE_FACTOR = F(.001)                              # :20
RADIANS = F(0.017453292519943295)


def aux_block(aux=None):
    """the sbx_aux_clouds block as a record of oracle/aux_sets.py: None = the defaults, a dict = the fields that differ from them,
    anything else = the bytes of a block (a ctypes structure of shaderbox_amd, a record)"""
    if aux is None or isinstance(aux, dict):
        return aux_sets.block("clouds", aux)
    return aux_sets.from_bytes("clouds", aux)


def _exp(x):
    return oracle().math("exp", np.ascontiguousarray(x, dtype=F))


def _pow(x, p):
    return oracle().math("pow", np.ascontiguousarray(x, dtype=F), F(p))


def clamp(x, lo, hi):                               # m_clamp
    return fmin(fmax(x, lo), hi)


def smoothstep(e0, e1, x):                          # m_smoothstep
    t = clamp((x - e0) / (e1 - e0), ZERO, ONE)
    return (t * t) * (F(3.) - TWO * t)


def mix(x, y, a):                                   # m_mix
    return x * (ONE - a) + y * a


def setup_camera(mouse):                            # :23-30
    eye = (ZERO, F(-.5), ZERO)
    a = _f(F(mouse[0]) * F(.5) * RADIANS).reshape(1)
    s, c = oracle().math("sin", a)[0], oracle().math("cos", a)[0]
    cols = ((c, ZERO, s), (ZERO, ONE, ZERO), (-s, ZERO, c))     # rotate_around_y, column by column (util.h:53-60)
    v = (ZERO, ZERO, F(-1))
    look_at = tuple((cols[0][k] * v[0] + cols[1][k] * v[1]) + cols[2][k] * v[2] for k in range(3))
    return eye, look_at


def render_sky_color(d, A):                         # :36-46
    sun_dir, sun_color = A["sun_dir"], A["sun_color"]
    sun_amount = fmax(dot(d, sun_dir), ZERO)
    t = ONE - d[1]
    lo, hi = (F(.0), F(.1), F(.4)), (F(.3), F(.6), F(.8))
    glare = fmin(_pow(sun_amount, 1500.0) * F(5.0), ONE)
    glow = fmin(_pow(sun_amount, 10.0) * F(.6), ONE)
    return [np.abs((mix(lo[k], hi[k], t) + sun_color[k] * glare) + sun_color[k] * glow) for k in range(3)]


def density_func(pos, A):                           # :62-86 over fbm = 4 octaves of noise_iq (:59, fbm.h)
    p = [(pos[k] * NOISE_FACTOR) * F(2.03) for k in range(3)]
    t, H = np.zeros_like(p[0]), F(.5)
    for _ in range(4):
        n = oracle().noise("noise_iq", np.stack(p, axis=-1))[:, 0]
        t = t + n * H
        p = [c * F(2.64) for c in p]
        H = H * F(.5)
    cov = ONE - A["cld_coverage"]
    return t * smoothstep(cov, cov + F(.0135), t)


def light_march(origin, A, dt):                     # :100-115 -> vol.transmittance
    L = A["sun_dir"]
    step = [L[k] * dt for k in range(3)]
    pos = [origin[k] + step[k] for k in range(3)]
    tr = np.ones_like(origin[0])
    for _ in range(int(A["illum_march_steps"])):
        density = density_func(pos, A)
        tr = tr * _exp(-density * A["sigma_scattering"] * dt)
        pos = [pos[k] + step[k] for k in range(3)]
    return tr


def render_clouds(build, d, eye, u_time, A):        # :153-202 -> radiance, alpha * smoothstep(0, .2, cutoff)
    n = d[0].size
    steps = int(A["cld_march_steps"])
    with np.errstate(all="ignore"):
        proj = [d[k] / d[1] for k in range(3)]
        wind = [(A["wind_dir"][k] * F(u_time)) * (ONE / NOISE_FACTOR) for k in range(3)]
        origin = [(eye[k] + proj[k] * F(150.)) + wind[k] for k in range(3)]
        dt = A["cld_thick"] / F(steps)
        sigma = A["sigma_scattering"]
        trans, radiance, alpha = np.ones(n, dtype=F), np.zeros(n, dtype=F), np.zeros(n, dtype=F)
        phase = None
        if build != "luminance":                    # volumetric.h:27-33 with hg_g = .2; the same for every step of a pixel
            mu = clamp(dot(A["sun_dir"], d), ZERO, ONE)
            phase = (ONE - HG_G * HG_G) / ((F(4.) + PI) * _pow(ONE + HG_G * HG_G - TWO * HG_G * mu, 1.5))
        alive = np.ones(n, dtype=bool)
        t = ZERO
        for i in range(steps):
            idx = np.nonzero(alive)[0]
            if idx.size == 0:
                break
            pos = [origin[k][idx] + t * proj[k][idx] for k in range(3)]
            t = t + dt
            density = density_func(pos, A)
            lit = ~(density < F(.005))              # integrate_volume :132
            li = idx[lit]
            if li.size:
                dl = density[lit]
                T_i = _exp(-dl * sigma * dt)
                trans[li] = trans[li] * T_i
                if build == "height":               # :98 with height = float(i) / float(cld_march_steps) (:183)
                    lum = _exp(_f(F(i) / F(steps)).reshape(1))[0] / TWO
                    illum = (lum * A["sun_power"]) * phase[li]
                else:
                    lum = light_march([p[lit] for p in pos], A, dt)
                    illum = lum if build == "luminance" else (lum * A["sun_power"]) * phase[li]
                radiance[li] = radiance[li] + (((dl * sigma) * illum) * trans[li]) * dt
                alpha[li] = alpha[li] + (ONE - T_i) * (ONE - alpha[li])
            alive[idx[alpha[idx] > F(.999)]] = False
        cutoff = dot(d, (ZERO, ONE, ZERO))
        return radiance, alpha * smoothstep(F(.0), F(.2), cutoff)


def main_image(build, width, height, u_time, fx, fy, aux=None, mouse=(0.0, 0.0)):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    assert build in BUILDS, build
    A = aux_block(aux)
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), FOV)
    eye, look_at = setup_camera(mouse)
    d = get_primary_ray(pcx, pcy, eye, look_at)
    with np.errstate(all="ignore"):
        sky = render_sky_color(d, A)                # render :204-218
        col = [s.copy() for s in sky]
        m = np.nonzero(~(dot(d, (ZERO, ONE, ZERO)) < F(0.05)))[0]
        if m.size:
            rad, a = render_clouds(build, [c[m] for c in d], eye, u_time, A)
            for k in range(3):
                col[k][m] = np.abs(mix(sky[k][m], rad, a))
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    for k in range(3):
        out[:, k] = _pow(col[k], F(1) / F(2.2))
    return out.reshape(shape + (4,))


def frame(build, width, height, u_time, aux=None, mouse=(0.0, 0.0)):
    """float32 [H, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre)"""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(build, width, height, u_time, fx, fy, aux, mouse)
fixture = functools.partial(builds_fixture, "clouds")     # tests/golden/clouds_builds/ decoded: tests/model_common.py
