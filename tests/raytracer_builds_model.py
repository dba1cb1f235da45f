"""The four builds of src/app_raytracer.h, which holds three compile-time switches, restated in numpy binary32 step by step in the
oracle's operation order (oracle/ref_apps.h AppRaytracer, oracle/ref_lib.h, oracle/ovec.h):
    "default"    the file as shipped                                                             SBX_APP_RAYTRACER
    "phong"      the `#if 0` of illuminate at :61 on: illum_blinn_phong (light.h:44-62, its `#else` branch,
                 the Phong specular) instead of illum_cook_torrance                              SBX_APP_RAYTRACER_PHONG
    "noshadow"   the `#if 1 // shadow ray` of render at :107 off: :108-121 are gone              SBX_APP_RAYTRACER_NOSHADOW
    "static"     the `#if 1` of setup_scene at :29 off: the Cornell box as cornell_box.h:71-85
                 puts it, u_time not read                                                        SBX_APP_RAYTRACER_STATIC
sin, cos, tan, exp and pow are the math spec's (Oracle.math); everything else is np.float32 arithmetic, one rounding per operation.
Vectorised over the pixels: every pixel runs both bounces' arithmetic and masks choose what it keeps.

The definition is pinned from two sides (tests/test_raytracer_builds_cpu.py): "default" equals the oracle in every bit, the other
three equal the frames and points that the edited reference header itself rendered (tests/golden/raytracer_builds/,
tools/make_golden_builds.py)."""
import functools

import numpy as np

from tests.model_common import F, ONE, RADIANS, TWO, ZERO, _f, _sincos, builds_fixture, dot, fmax, fmin, get_primary_ray, oracle, point_cam, same_bits  # noqa: F401

BUILDS = ("default", "phong", "noshadow", "static")
APP_OF = {"default": "raytracer", "phong": "raytracer_phong", "noshadow": "raytracer_noshadow", "static": "raytracer_static"}
PI = F(3.14159265359)                               # def.h:51
BIAS = F(1e-4)                                      # def.h:57
MAX_DIST = F(1e8)                                   # def.h:77
CB = F(2.)                                          # cb_plane_dist cornell_box.h:63
AMBIENT = F(.01)                                    # light.h:16


def _math(fn, x, y=None):
    x = np.ascontiguousarray(x, dtype=F)
    return oracle().math(fn, x.ravel(), None if y is None else F(y)).reshape(x.shape)


def fov():                                          # app_raytracer.h:138: tan(radians(30.))
    return _math("tan", _f(F(30.) * RADIANS).reshape(1))[0]


def scene(build, u_time):
    """setup_scene (:18-36) over setup_cornell_box (cornell_box.h:39-87): planes [(n, d, mat)] in array order, spheres
    [(origin, radius, mat)], the eight material slots as arrays indexed by id, lights[0].L"""
    planes = [((ZERO, F(-1), ZERO), ZERO, 1), ((ZERO, ZERO, F(-1)), -CB, 1), ((ZERO, ZERO, ONE), CB, 1),
              ((ZERO, ONE, ZERO), TWO * CB, 1), ((ONE, ZERO, ZERO), CB, 2), ((F(-1), ZERO, ZERO), -CB, 3)]
    base = np.zeros((8, 3), dtype=F)                # material.h:17: zero-initialised slots
    rough, ior, refl = np.zeros(8, dtype=F), np.zeros(8, dtype=F), np.zeros(8, dtype=F)
    base[0], rough[0], ior[0] = (1., 1., 1.), 0., 1.
    for i, (c, r) in enumerate([((0.7913, 0.7913, 0.7913), .5), ((0.6795, 0.0612, 0.0529), .5), ((0.1878, 0.1274, 0.4287), .5),
                                ((0.95, 0.64, 0.54), .1), ((1., 0.77, 0.345), .05)], start=1):
        base[i], rough[i], ior[i] = c, r, 1.
    refl[4] = refl[5] = 1.
    ior[5] = 1.333
    left = [F(0.75), ONE, F(-0.75)]
    right = [F(-0.75), F(0.75), F(0.75)]
    light = [ZERO, TWO * CB - F(0.2), ZERO]
    if build != "static":                           # :29-35
        t = _f(u_time).reshape(1)
        with np.errstate(all="ignore"):
            s, c = _math("sin", t)[0], _math("cos", t)[0]
            left = [left[0] + ZERO, left[1] + np.abs(s), left[2] + (c + ONE)]
        right[2] = ZERO
        light[2] = F(1.5)
    spheres = [((ZERO, F(2.5) * CB + F(0.4), ZERO), F(1.5), 0), (tuple(left), F(0.75), 4), (tuple(right), F(0.75), 5)]
    return dict(planes=planes, spheres=spheres, base=base, rough=rough, ior=ior, refl=refl, light=tuple(light))


def setup_camera(width, height, mouse):             # :38-44
    with np.errstate(all="ignore"):
        mx = F(mouse[0])
        m = ZERO if mx < BIAS else TWO * (F(width) / mx) - ONE
        s, c = _sincos(m * F(30.))
        cols = ((c, ZERO, s), (ZERO, ONE, ZERO), (-s, ZERO, c))          # rotate_around_y, column by column (util.h:53-60)
        v = (ZERO, CB, F(2.333) * CB)
        eye = tuple((cols[0][k] * v[0] + cols[1][k] * v[1]) + cols[2][k] * v[2] for k in range(3))
    return eye, (ZERO, CB, ZERO)


def normalize(v):                                   # oracle/ovec.h:69-70
    n = np.sqrt(dot(v, v))
    return [v[0] / n, v[1] / n, v[2] / n]


def trace(S, ro, rd, mat_to_ignore):                # raytrace_iteration :70-86 -> t, material id, normal, origin
    n = rd[0].shape
    t = np.full(n, MAX_DIST + F(1e1), dtype=F)      # no_hit def.h:78-83
    mat = np.full(n, -1, dtype=np.int32)
    nor = [np.zeros(n, dtype=F) for _ in range(3)]
    org = [np.zeros(n, dtype=F) for _ in range(3)]
    for pn, pd, pm in S["planes"]:                  # intersect_plane intersect.h:61-77
        denom = dot(pn, rd)
        tt = dot([pd - ro[k] for k in range(3)], pn) / denom
        ok = ~(denom < F(1e-6)) & ~((tt < ZERO) | (tt > t))
        front = denom < ZERO                        # faceforward(N, I, Nref = N) util.h:85-93
        t = np.where(ok, tt, t)
        mat = np.where(ok, pm, mat)
        for k in range(3):
            org[k] = np.where(ok, ro[k] + rd[k] * tt, org[k])
            nor[k] = np.where(ok, np.where(front, pn[k], -pn[k]), nor[k])
    for so, sr, sm in S["spheres"]:                 # intersect_sphere intersect.h:7-33
        if sm == mat_to_ignore:
            continue
        rc = [so[k] - ro[k] for k in range(3)]
        radius2 = sr * sr
        tca = dot(rc, rd)
        d2 = dot(rc, rc) - tca * tca
        thc = np.sqrt(radius2 - d2)
        t0, t1 = tca - thc, tca + thc
        t0 = np.where(t0 < ZERO, t1, t0)
        ok = ~(tca < ZERO) & ~(d2 > radius2) & ~(t0 > t)
        t = np.where(ok, t0, t)
        mat = np.where(ok, sm, mat)
        for k in range(3):
            impact = ro[k] + rd[k] * t0
            org[k] = np.where(ok, impact, org[k])
            nor[k] = np.where(ok, (impact - so[k]) / sr, nor[k])
    return t, mat, nor, org


def fresnel_factor(n1, n2, VdotH):                  # util_optics.h:5-14
    Rn = (n1 - n2) / (n1 + n2)
    R0 = Rn * Rn
    Fc = ONE - VdotH
    return R0 + (ONE - R0) * ((((Fc * Fc) * Fc) * Fc) * Fc)


def material(S, mat):
    """get_material (material.h:19-36): the slot for an id of 0..7, the zero-initialised material for any other"""
    inside = (mat >= 0) & (mat < 8)
    i = np.where(inside, mat, 0)
    pick = lambda a: np.where(inside, a[i], ZERO)   # noqa: E731
    return [pick(S["base"][:, k]) for k in range(3)], pick(S["rough"]), pick(S["ior"]), pick(S["refl"])


def illum_cook_torrance(V, L, nor, base, rough, ior):   # light.h:64-92
    H = normalize([L[k] + V[k] for k in range(3)])
    NdotL, NdotH, NdotV, VdotH = dot(nor, L), dot(nor, H), dot(nor, V), dot(V, H)
    geo_a = (TWO * NdotH * NdotV) / VdotH
    geo_b = (TWO * NdotH * NdotL) / VdotH
    geo_term = fmin(ONE, fmin(geo_a, geo_b))
    rough_sq = rough * rough
    rough_a = ONE / (rough_sq * NdotH * NdotH * NdotH * NdotH)
    rough_exp = (NdotH * NdotH - ONE) / (rough_sq * NdotH * NdotH)
    rough_term = rough_a * _math("exp", rough_exp)
    fresnel_term = fresnel_factor(ONE, ior, VdotH)
    specular = (geo_term * rough_term * fresnel_term) / (PI * NdotV * NdotL)
    return [fmax(ZERO, NdotL) * (specular + base[k]) for k in range(3)]


def illum_blinn_phong(V, L, nor, base):             # light.h:44-62, the `#else` (Phong) branch of :53
    d = fmax(ZERO, dot(L, nor))
    diffuse = [d * base[k] for k in range(3)]
    I = [-L[k] for k in range(3)]                   # noqa: E741  reflect(-L, N), util_optics.h:17-22: the negated zeros stay
    s = TWO * dot(nor, I)
    R = [I[k] - s * nor[k] for k in range(3)]
    specular = _math("pow", fmax(ZERO, dot(R, V)), 50.) * ONE
    return [diffuse[k] + specular for k in range(3)]


def illuminate(build, S, eye, mat, nor, org):       # :46-68
    base, rough, ior, _ = material(S, mat)
    V = normalize([eye[k] - org[k] for k in range(3)])
    L = normalize([S["light"][k] - org[k] for k in range(3)])      # get_light_direction, LIGHT_POINT (light.h:18-27)
    lit = illum_blinn_phong(V, L, nor, base) if build == "phong" else illum_cook_torrance(V, L, nor, base, rough, ior)
    debug = mat == 0                                # mat_debug: materials[mat_debug].base_color
    return [np.where(debug, S["base"][0, k], AMBIENT + lit[k]) for k in range(3)]


def render(build, S, eye, rd):                      # :88-136
    n = rd[0].shape
    color = [np.zeros(n, dtype=F) for _ in range(3)]
    accum = [np.ones(n, dtype=F) for _ in range(3)]
    ro = [np.full(n, eye[k], dtype=F) for k in range(3)]
    rd = list(rd)
    active = np.ones(n, dtype=bool)
    for i in range(2):
        t, mat, nor, org = trace(S, ro, rd, -1)
        miss = active & (t >= MAX_DIST)
        live = active & ~miss
        f = fresnel_factor(ONE, ONE, dot(nor, [-rd[k] for k in range(3)]))
        ill = illuminate(build, S, eye, mat, nor, org)
        for k in range(3):
            color[k] = np.where(miss, color[k] + accum[k] * ZERO, color[k])              # background :13-16
            color[k] = np.where(live, color[k] + ((ONE - f) * accum[k]) * ill[k], color[k])
        if i == 0 and build != "noshadow":          # shadow ray :108-121
            line = [S["light"][k] - org[k] for k in range(3)]
            sdir = normalize(line)
            st = trace(S, [org[k] + sdir[k] * BIAS for k in range(3)], sdir, 0)[0]
            dark = live & (st < np.sqrt(dot(line, line)))
            for k in range(3):
                color[k] = np.where(dark, color[k] * F(0.1), color[k])
        refl = live & (material(S, mat)[3] > ZERO)
        s = TWO * dot(rd, nor)                      # reflect(hit.normal, ray.direction): arguments swapped in the reference (:127)
        rdir = normalize([nor[k] - s * rd[k] for k in range(3)])
        for k in range(3):
            accum[k] = np.where(refl, accum[k] * f, accum[k])
            ro[k] = np.where(refl, org[k] + rdir[k] * BIAS, ro[k])
            rd[k] = np.where(refl, rdir[k], rd[k])
        active = refl
    return color


def main_image(build, width, height, u_time, fx, fy, mouse=(0.0, 0.0)):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    assert build in BUILDS, build
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), fov())
    eye, look_at = setup_camera(width, height, mouse)
    rd = get_primary_ray(pcx, pcy, eye, look_at)
    with np.errstate(all="ignore"):
        color = render(build, scene(build, u_time), eye, rd)
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    for k in range(3):
        out[:, k] = _math("pow", color[k], F(1) / F(2.2))
    return out.reshape(shape + (4,))


def frame(build, width, height, u_time, mouse=(0.0, 0.0)):
    """float32 [H, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre)"""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(build, width, height, u_time, fx, fy, mouse)
fixture = functools.partial(builds_fixture, "raytracer")     # tests/golden/raytracer_builds/ decoded: tests/model_common.py
