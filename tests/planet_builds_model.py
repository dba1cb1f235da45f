"""numpy restatement of the four builds of src/app_planet.h: SBX_APP_PLANET ("default", as shipped), SBX_APP_PLANET_CLOSEUP ("closeup",
the `#if 0` of setup_camera at :51 turned to `#if 1`: eye and look_at of :52-53), SBX_APP_PLANET_CLOUDLESS ("cloudless", the
`#define CLOUDS` of :63 gone: no clouds_march, no clouds_shadow_march, `cloud` the zeros of the static object) and
SBX_APP_PLANET_UNLIT ("unlit", the `#define LIGHT` of :249 gone: N = w_normal.y, ocean = water, no setup_lights); include/sbx.h,
DESIGN.md §5.16.

The CPU oracle renders the shipped build only and is not to grow, so the GPU tests of the three other builds compare against this
module.  It is pinned from two sides (tests/test_planet_builds_cpu.py): build "default" equals Oracle.render("planet") in every bit —
which covers everything the four builds share: camera arithmetic, the atmosphere test, both terrain maps, the terrain march, the cloud
integrator and its two marches, illuminate, background, epilogue — and the other three equal frames and points that the reference
header itself rendered with the one line edited (tests/golden/planet_builds/, tools/make_golden_builds.py), NaN pixels
included.

mainImage -> render -> sdf_terrain_map / clouds_march / illuminate / clouds_shadow_march, vectorised over pixels, in binary32 step
by step in the oracle's operation order (oracle/ovec.h: dot = (x x + y y) + z z, normalize = three divisions by sqrtf, M * v =
(c0 v.x + c1 v.y) + c2 v.z; oracle/sbx_math_ref.h: min / max as compare-and-select, mix = x (1 - a) + y a, smoothstep's division by
e1 - e0), every value an explicit np.float32.  sin, cos, tan, exp, pow and noise_iq are the oracle's (Oracle.math, Oracle.noise).
The vector algebra and the camera are tests/model_common.py's; matrices are tests/vinyl_builds_model.py's and tests/egg_builds_model.py's.
"""
import functools

import numpy as np

from tests.egg_builds_model import clamp, mat_vec, mix
from tests.model_common import F, ONE, RADIANS, TWO, ZERO, _f, builds_fixture, dot, fmax, get_primary_ray, normalize, oracle, point_cam
from tests.vinyl_builds_model import mat_mat, rotate_around_x, rotate_around_y

BUILDS = ("default", "closeup", "cloudless", "unlit")
APP_OF = {"default": "planet", "closeup": "planet_closeup", "cloudless": "planet_cloudless", "unlit": "planet_unlit"}
# setup_camera :47-58: (eye, look_at); the `#if` pair for closeup
CAMERA = {b: ((F(0), F(0), F(-2.5)), (F(0), F(0), F(2))) for b in BUILDS}
CAMERA["closeup"] = ((F(.0), F(0), F(-1.93)), (F(-.1), F(.9), F(2)))
MAX_HEIGHT = F(.4)                                  # :20
MAX_RAY_DIST = MAX_HEIGHT * F(4.)                   # :21
TERR_STEPS, TERR_EPS = 120, F(.005)                 # :165-166
ABSORB = F(30.034)                                  # :68
HIT_T = F(F(1e8) + F(1e1))                          # no_hit.t def.h:78-83


def _math(fn, x, y=None):
    x = np.ascontiguousarray(x, dtype=F)
    return oracle().math(fn, x.ravel(), None if y is None else F(y)).reshape(x.shape)


def fov():                                          # :369: tan(radians(30.))
    return _math("tan", _f(F(30.) * RADIANS).reshape(1))[0]


def smoothstep(e0, e1, x):                          # m_smoothstep
    t = clamp((x - e0) / (e1 - e0), ZERO, ONE)
    return (t * t) * (F(3.) - TWO * t)


def band(start, peak, end, t):                      # util.h:103-112
    return smoothstep(start, peak, t) * (ONE - smoothstep(peak, end, t))


def length3(v):
    return np.sqrt(dot(v, v))


def transpose(m):                                   # util.h:24-33; m = columns
    return tuple((m[0][k], m[1][k], m[2][k]) for k in range(3))


def noise(p):
    return oracle().noise("noise_iq", np.stack(p, axis=-1))[:, 0]


def fbm(p, octaves, lacunarity, init_gain, gain, basis):      # fbm.h:6
    p = list(p)
    H = F(init_gain)
    t = np.zeros_like(p[0])
    for _ in range(octaves):
        t = t + basis(noise(p)) * H
        p = [c * F(lacunarity) for c in p]
        H = H * F(gain)
    return t


def _noise(n):                                      # :9
    return n


def _anoise(n):                                     # :65
    return np.abs(n * TWO - ONE)


def _rnoise(n):                                     # :167
    return ONE - np.abs(n * TWO - ONE)


def sdf_terrain_map(pos, octaves=3):
    """sdf_terrain_map (:175-186; octaves = 3) and sdf_terrain_map_detail (:188-199; 7) -> (df.x, df.y)"""
    h0 = fbm([c * F(2.0987) for c in pos], octaves, 2.0244, .454, .454, _noise)
    n0 = smoothstep(F(.35), F(1.), h0)
    off = (F(1.9489), F(2.435), F(.5483))
    h1 = fbm([pos[k] * F(1.50987) + off[k] for k in range(3)], octaves, 2.0244, .454, .454, _rnoise)
    n1 = smoothstep(F(.6), F(1.), h1)
    n = n0 + n1
    return length3(pos) - ONE - n * MAX_HEIGHT, n / MAX_HEIGHT


def sdf_terrain_normal(p):                          # :201-212
    e = F(0.001)

    def d(k, sign):
        dt = [ZERO, ZERO, ZERO]
        dt[k] = e
        q = [p[c] + dt[c] if sign > 0 else p[c] - dt[c] for c in range(3)]
        return sdf_terrain_map(q, 7)[0]

    return normalize((d(0, 1) - d(0, -1), d(1, 1) - d(1, -1), d(2, 1) - d(2, -1)))


def setup_lights(L, normal):                        # :217-236
    zero = np.zeros_like(normal[0])
    key = fmax(zero, dot(L, normal))
    c_L = (F(7), F(5), F(3))
    diffuse = [ZERO + key * c_L[k] for k in range(3)]
    hemi = clamp(F(.25) + F(.5) * normal[1], ZERO, ONE)
    fill = (F(.4), F(.6), F(.8))
    diffuse = [diffuse[k] + (hemi * fill[k]) * F(.2) for k in range(3)]
    amb = clamp(F(.12) + F(.8) * fmax(zero, dot((-L[0], -L[1], -L[2]), normal)), ZERO, ONE)
    rev = (F(.4), F(.5), F(.6))
    return [diffuse[k] + amb * rev[k] for k in range(3)]


def illuminate(build, pos, rot, h):                 # :238-298 -> [3] arrays
    w_normal = normalize(pos)
    if build != "unlit":
        normal = sdf_terrain_normal(pos)
        N = dot(normal, w_normal)
    else:
        N = w_normal[1]
    c_water, c_grass, c_beach = (F(.015), F(.110), F(.455)), (F(.086), F(.132), F(.018)), (F(.153), F(.172), F(.121))
    c_rock, c_snow = (F(.080), F(.050), F(.030)), (F(.600), F(.600), F(.600))
    l_water, l_shore, l_grass, l_rock = F(.05), F(.17), F(.211), F(.351)
    s = smoothstep(F(.4), F(1.), h)
    a = smoothstep(ONE - F(.3) * s, ONE - F(.2) * s, N)
    rock = [mix(c_rock[k], c_snow[k], a) for k in range(3)]
    a = smoothstep(l_grass, l_rock, h)
    grass = [mix(c_grass[k], rock[k], a) for k in range(3)]
    a = smoothstep(l_shore, l_grass, h)
    shoreline = [mix(c_beach[k], grass[k], a) for k in range(3)]
    a = smoothstep(ZERO, l_water, h)
    water = [mix(c_water[k] / TWO, c_water[k], a) for k in range(3)]
    if build != "unlit":
        L = mat_vec(rot, normalize((ONE, ONE, ZERO)))
        lit = setup_lights(L, normal)
        shoreline = [shoreline[k] * lit[k] for k in range(3)]
        lit = setup_lights(L, w_normal)
        ocean = [lit[k] * water[k] for k in range(3)]
    else:
        ocean = water
    a = smoothstep(l_water, l_shore, h)
    return [mix(ocean[k], shoreline[k], a) for k in range(3)]


def clouds_map(c, t_step):
    """clouds_map (:102-119) + integrate_volume (:79-100) on the sampler c = dict(pos, height, tr, radiance, alpha), in place"""
    off = (F(.35), F(13.35), F(2.67))
    dens = fbm([c["pos"][k] * F(3.2343) + off[k] for k in range(3)], 4, 2.0276, .5, .5, _anoise)
    cov, fuzzy = F(.29475675), F(.0335)
    dens = dens * smoothstep(cov, cov + fuzzy, dens)
    dens = dens * band(F(.2), F(.35), F(.65), c["height"])
    T_i = _math("exp", -ABSORB * dens * t_step)
    c["tr"] = c["tr"] * T_i
    c["radiance"] = c["radiance"] + dens * (_math("exp", c["height"]) / F(.055)) * c["tr"] * t_step
    c["alpha"] = c["alpha"] + (ONE - T_i) * (ONE - c["alpha"])


def clouds_march(origin, rd, max_travel, rot_cloud):
    """clouds_march (:121-141) on construct_volume(origin) -> (radiance, alpha)"""
    n = rd[0].size
    steps = 75
    t_step = MAX_RAY_DIST / F(steps)
    t = np.zeros(n, dtype=F)
    tr, radiance, alpha = np.ones(n, dtype=F), np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    act = np.arange(n)
    for _ in range(steps):
        act = act[~((t[act] > max_travel[act]) | (alpha[act] >= ONE))]
        if act.size == 0:
            break
        o = [origin[k][act] + t[act] * rd[k][act] for k in range(3)]
        pos = mat_vec(rot_cloud, o)
        c = {"pos": pos, "height": (length3(pos) - ONE) / MAX_HEIGHT, "tr": tr[act], "radiance": radiance[act], "alpha": alpha[act]}
        t[act] = t[act] + t_step
        clouds_map(c, t_step)
        tr[act], radiance[act], alpha[act] = c["tr"], c["radiance"], c["alpha"]
    return radiance, alpha


def clouds_shadow_march(origin, direction, rot_cloud):          # :143-160 on construct_volume(origin) -> alpha
    n = origin[0].size
    steps = 5
    t_step = MAX_HEIGHT / F(steps)
    t = F(0.)
    c = {"tr": np.ones(n, dtype=F), "radiance": np.zeros(n, dtype=F), "alpha": np.zeros(n, dtype=F)}
    for _ in range(steps):
        o = [origin[k] + t * direction[k] for k in range(3)]
        c["pos"] = mat_vec(rot_cloud, o)
        c["height"] = (length3(c["pos"]) - ONE) / MAX_HEIGHT
        t = t + t_step
        clouds_map(c, t_step)
    return c["alpha"]


def background(rd):                                 # :23-41 -> [3] arrays
    sun_color = (F(1.), F(.9), F(.55))
    sun_amount = clamp((rd[0] * ZERO + rd[1] * ZERO) + rd[2] * ONE, ZERO, ONE)
    lo, hi = (F(.0), F(.05), F(.2)), (F(.15), F(.3), F(.4))
    a = ONE - rd[1]
    glare = clamp(_math("pow", sun_amount, 30.0) * F(5.0), ZERO, ONE)
    glow = clamp(_math("pow", sun_amount, 10.0) * F(.6), ZERO, ONE)
    return [np.abs((mix(lo[k], hi[k], a) + sun_color[k] * glare) + sun_color[k] * glow) for k in range(3)]


# ---- the pixel -----------------------------------------------------------------------------------------------------------

def render(build, u_time, ro, rd, parts=None):
    """render (:303-367) for rays (ro, rd[3][n]) -> rgb[n, 3].  parts: a dict that receives atm (the ray meets the atmosphere shell),
    ground (df.x < TERR_EPS at :349), alpha (cloud.alpha after the view march; the static object's 0 in the cloudless build) and
    shadow (the value of `shadow` at :363; 1 where there is no ground hit)."""
    n = rd[0].size
    clouds = build != "cloudless"
    with np.errstate(all="ignore"):
        t = F(u_time)
        rot_y = rotate_around_y(27.)
        rot = mat_mat(rotate_around_x(t * F(-12.)), rot_y)
        rot_cloud = mat_mat(rotate_around_x(t * F(8.)), rot_y)
        # intersect_sphere(eye, {planet.origin, 1 + max_height}, no_hit)   intersect.h:7-33
        radius = ONE + MAX_HEIGHT
        rc = (ZERO - ro[0], ZERO - ro[1], ZERO - ro[2])
        radius2 = radius * radius
        tca = dot(rc, rd)
        d2 = dot(rc, rc) - tca * tca
        thc = np.sqrt(radius2 - d2)
        t0 = tca - thc
        t0 = np.where(t0 < ZERO, tca + thc, t0)
        atm = ~(tca < ZERO) & ~(d2 > radius2) & ~(t0 > HIT_T)
        rgb = np.zeros((n, 3), dtype=F)
        miss = np.flatnonzero(~atm)
        if miss.size:
            rgb[miss] = np.stack(background([rd[k][miss] for k in range(3)]), axis=1)
        ground = np.zeros(n, dtype=bool)
        alpha_out = np.zeros(n, dtype=F)
        shadow_out = np.ones(n, dtype=F)
        ia = np.flatnonzero(atm)
        if ia.size:
            m = ia.size
            d = [rd[k][ia] for k in range(3)]
            origin = [ro[k] + d[k] * t0[ia] for k in range(3)]
            # terrain march :323-342
            tt = np.zeros(m, dtype=F)
            dfx, dfy = np.ones(m, dtype=F), np.full(m, MAX_HEIGHT, dtype=F)
            pos = [np.zeros(m, dtype=F) for _ in range(3)]
            max_cld = np.full(m, MAX_RAY_DIST, dtype=F)
            act = np.arange(m)
            for _ in range(TERR_STEPS):
                act = act[~(tt[act] > MAX_RAY_DIST)]
                if act.size == 0:
                    break
                o = [origin[k][act] + tt[act] * d[k][act] for k in range(3)]
                p = mat_vec(rot, o)
                x, y = sdf_terrain_map(p)
                for k in range(3):
                    pos[k][act] = p[k]
                dfx[act], dfy[act] = x, y
                hit = x < TERR_EPS
                max_cld[act[hit]] = tt[act[hit]]
                go = ~hit
                tt[act[go]] = tt[act[go]] + x[go] * F(.4567)
                act = act[go]
            if clouds:                              # :344-347
                radiance, alpha = clouds_march(origin, d, max_cld, rot_cloud)
            else:                                   # `cloud` is the static object nothing has written
                radiance, alpha = np.zeros(m, dtype=F), np.zeros(m, dtype=F)
            alpha_out[ia] = alpha
            g = dfx < TERR_EPS                      # :349
            ground[ia] = g
            ig = np.flatnonzero(g)
            if ig.size:
                ph = [pos[k][ig] for k in range(3)]
                c_terr = illuminate(build, ph, rot, dfy[ig])
                shadow = np.ones(ig.size, dtype=F)
                if clouds:                          # :355-361
                    lp = mat_vec(transpose(rot), ph)
                    sa = clouds_shadow_march(lp, normalize(lp), rot_cloud)
                    shadow = mix(F(.7), F(1.), np.where(F(0.33) < sa, ZERO, ONE).astype(F))
                shadow_out[ia[ig]] = shadow
                for k in range(3):
                    rgb[ia[ig], k] = np.abs(mix(c_terr[k] * shadow, radiance[ig], alpha[ig]))
            isky = np.flatnonzero(~g)
            if isky.size:                           # :364-366
                bg = background([d[k][isky] for k in range(3)])
                for k in range(3):
                    rgb[ia[isky], k] = np.abs(mix(bg[k], radiance[isky], alpha[isky]))
        if parts is not None:
            parts.update(atm=atm, ground=ground, alpha=alpha_out, shadow=shadow_out)
    return rgb


def main_image(build, width, height, u_time, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]; parts as render's, flat in the order of fx.ravel()"""
    assert build in BUILDS, build
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    eye, look_at = CAMERA[build]
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), fov())
    rd = get_primary_ray(pcx, pcy, eye, look_at)
    rgb = render(build, u_time, eye, rd, parts)
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    out[:, :3] = _math("pow", np.ascontiguousarray(rgb), F(1) / F(2.2))
    return out.reshape(shape + (4,))


def frame(build, width, height, u_time, mouse=(0.0, 0.0), parts=None):
    """float32 [H, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre).  u_mouse is not read.  parts: flat, row by row."""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(build, width, height, u_time, fx, fy, parts)


fixture = functools.partial(builds_fixture, "planet")     # tests/golden/planet_builds/ decoded: tests/model_common.py
