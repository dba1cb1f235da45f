"""numpy restatement of SBX_APP_PLANET_WORLD (include/sbx.h): src/app_planet.h as shipped (CLOUDS and LIGHT defined)
with every number the block sbx_aux_planet_world carries read from it — the definition of the app.  tests/planet_builds_model.py's
functions (whose helpers, fBm, background and operation order it imports) with the literals taken from a world; everything derived is
binary32 arithmetic on the block's values in the header's order: max_ray_dist = max_height * 4, the atmosphere's radius 1 + max_height,
t_step = max_ray_dist / float(cloud_steps) and max_height / float(shadow_steps), c_water / 2, cld_coverage + cld_fuzzy.  A world is a
dict of the struct's fields; tier_of restates the host's choice of kernel (csrc/sbx_frames.hip planet_world_tier, planet_world_tame,
planet_world_camera_tame).  tests/test_planet_world_cpu.py pins the default world to planet_builds_model's shipped frame, which the
oracle pins to the reference."""
import os

import numpy as np

from tests import planet_builds_model as P
from tests.egg_builds_model import clamp, mat_vec, mix
from tests.model_common import F, ONE, TWO, ZERO, _f, dot, fmax, get_primary_ray, normalize, point_cam, same_bits
from tests.planet_builds_model import _anoise, _math, _noise, _rnoise, background, fbm, length3, smoothstep, transpose
from tests.vinyl_builds_model import mat_mat, rotate_around_x, rotate_around_y

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZE, POINTS = (64, 36), 64
INT_FIELDS = ("terr_steps", "cloud_steps", "shadow_steps")
FIELDS = ("eye", "fov", "look_at", "tilt_deg", "sun_dir", "spin_deg", "key_color", "cloud_spin_deg", "terrain_offset", "max_height",
          "cloud_offset", "cld_coverage", "band", "cld_fuzzy", "c_water", "l_water", "c_grass", "l_shore", "c_beach", "l_grass", "c_rock",
          "l_rock", "c_snow", "absorb", "cloud_light", "terr_steps", "cloud_steps", "shadow_steps", "reserved")
CAMERA_FIELDS = ("eye", "fov", "look_at")
LITERAL_FREE = CAMERA_FIELDS + ("tilt_deg", "spin_deg", "cloud_spin_deg", "sun_dir")     # what a literal-tier block may change
LITERAL, RUNTIME, PLAIN = "literal", "run-time", "plain"
WORDS = 56                                            # 224 bytes


def _vec(v):
    return tuple(F(c) for c in v)


def default_world(u_time):
    """the header's numbers with the two spins of u_time: sbx_planet_world_default"""
    t = F(u_time)
    with np.errstate(all="ignore"):
        spin, cloud_spin = t * F(-12.), t * F(8.)
    return dict(eye=_vec((0, 0, -2.5)), fov=P.fov(), look_at=_vec((0, 0, 2)), tilt_deg=F(27.),
                sun_dir=_vec(normalize((ONE, ONE, ZERO))), spin_deg=spin, key_color=_vec((7, 5, 3)), cloud_spin_deg=cloud_spin,
                terrain_offset=_vec((1.9489, 2.435, .5483)), max_height=F(.4), cloud_offset=_vec((.35, 13.35, 2.67)),
                cld_coverage=F(.29475675), band=_vec((.2, .35, .65)), cld_fuzzy=F(.0335),
                c_water=_vec((.015, .110, .455)), l_water=F(.05), c_grass=_vec((.086, .132, .018)), l_shore=F(.17),
                c_beach=_vec((.153, .172, .121)), l_grass=F(.211), c_rock=_vec((.080, .050, .030)), l_rock=F(.351),
                c_snow=_vec((.600, .600, .600)), absorb=F(30.034), cloud_light=F(.055), terr_steps=120, cloud_steps=75, shadow_steps=5,
                reserved=(0, 0, 0, 0))


def world(u_time=0., **fields):
    """default_world(u_time) with the named fields replaced, each float rounded to binary32 once"""
    W = default_world(u_time)
    for k, v in fields.items():
        assert k in FIELDS, k
        W[k] = int(v) if k in INT_FIELDS else tuple(int(c) for c in v) if k == "reserved" else _vec(v) if isinstance(W[k], tuple) else F(v)
    return W


def block(W):
    """the 224 bytes of sbx_aux_planet_world as 56 words (uint32)"""
    out = []
    for k in FIELDS:
        if k in INT_FIELDS:
            out.append(np.array([W[k]], dtype=np.int32).view(np.uint32))
        elif k == "reserved":
            out.append(np.array(W[k], dtype=np.uint32))
        else:
            out.append(np.array(list(W[k]) if isinstance(W[k], tuple) else [W[k]], dtype=F).view(np.uint32))
    out = np.concatenate(out)
    assert out.shape == (WORDS,)
    return out


def of_block(words):
    """block()'s inverse"""
    words = np.asarray(words, dtype=np.uint32)
    W, at = {}, 0
    ref = default_world(0.)
    for k in FIELDS:
        n = len(ref[k]) if isinstance(ref[k], tuple) else 1
        w = words[at:at + n]
        at += n
        W[k] = int(w.view(np.int32)[0]) if k in INT_FIELDS else tuple(int(c) for c in w) if k == "reserved" else \
            tuple(w.view(F)) if isinstance(ref[k], tuple) else w.view(F)[0]
    return W


def as_aux(W):
    """the block as the ctypes struct the Python binding takes (shaderbox_amd.PlanetWorld)"""
    import ctypes

    import shaderbox_amd
    a = shaderbox_amd.PlanetWorld()
    assert ctypes.sizeof(a) == 4 * WORDS
    ctypes.memmove(ctypes.byref(a), block(W).tobytes(), 4 * WORDS)
    return a


# The fixture worlds: together every field differs from the default in at least one of them (test_planet_world_cpu.py asserts it).
# orbit moves camera, angles and sun only (the literal tier); the other four restate numbers (the run-time tier, tame).
T0 = .37
WORLDS = {
    "orbit": world(T0, eye=(1.6, .9, -2.1), look_at=(.1, -.05, .3), fov=.7, tilt_deg=-40., spin_deg=63., cloud_spin_deg=-21.,
                   sun_dir=(-.6, .3, .74)),
    "recoloured": world(T0, c_water=(.30, .07, .02), c_grass=(.20, .05, .22), c_beach=(.40, .36, .10), c_rock=(.10, .10, .14),
                        c_snow=(.55, .75, .80), l_water=.08, l_shore=.2, l_grass=.3, l_rock=.5, key_color=(3, 5, 8)),
    "overcast": world(T0, cld_coverage=.22, cld_fuzzy=.08, band=(.1, .3, .8), absorb=18.5, cloud_light=.09, cloud_offset=(4.5, -2.25, 7.),
                      cloud_steps=48, shadow_steps=7),
    "alpine": world(T0, max_height=.55, terrain_offset=(-3.1, .7, 5.9), terr_steps=90),
    "landing": world(T0, eye=(.35, 1.22, -.3), look_at=(-.5, 1.05, .9), fov=.9, spin_deg=10., max_height=.3, cld_coverage=.27),
}
POINT_SEEDS = {"orbit": 401, "recoloured": 402, "overcast": 403, "alpine": 404, "landing": 405}


# ---- the host's choice of kernel ----------------------------------------------------------------------------------------------------

def _same(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=F).view(np.uint32), np.asarray(b, dtype=F).view(np.uint32)))


def _in(v, lo, hi):
    with np.errstate(all="ignore"):
        return bool(F(v) >= F(lo)) and bool(F(v) <= F(hi))


def _zero_or_mag(v, lo, hi):
    return bool(F(v) == 0) or _in(np.abs(F(v)), lo, hi)


def rotations(W):
    """(rot, rot_cloud) :307-309"""
    with np.errstate(all="ignore"):
        rot_y = rotate_around_y(F(W["tilt_deg"]))
        return mat_mat(rotate_around_x(F(W["spin_deg"])), rot_y), mat_mat(rotate_around_x(F(W["cloud_spin_deg"])), rot_y)


def _orthonormal(m):
    c = [[float(x) for x in col] for col in m]
    for i in range(3):
        for j in range(i, 3):
            d = sum(c[i][k] * c[j][k] for k in range(3))
            if not abs(d - (1.0 if i == j else 0.0)) <= 1e-5:
                return False
    return True


def rotations_tame(W):
    rot, rot_cloud = rotations(W)
    return all(_in(np.abs(F(W[k])), 0, 1e9) for k in ("tilt_deg", "spin_deg", "cloud_spin_deg")) and _orthonormal(rot) and _orthonormal(rot_cloud)


def tame(W):
    """planet_world_tame: the domain of k_planet_world<true>'s guarded forms (csrc/kern_planet_world.hip)"""
    e20 = F(2.0 ** -20)
    with np.errstate(all="ignore"):
        if not _in(W["max_height"], .02, 2.):
            return False
        for k in range(3):
            if not _in(np.abs(W["terrain_offset"][k]), 0, 64) or not _in(np.abs(W["cloud_offset"][k]), 0, 64):
                return False
            if not _zero_or_mag(W["band"][k], e20, 4):
                return False
        if not _in(W["band"][1] - W["band"][0], e20, 8) or not _in(W["band"][2] - W["band"][1], e20, 8):
            return False
        if not _zero_or_mag(W["cld_coverage"], e20, 4):
            return False
        hi = W["cld_coverage"] + W["cld_fuzzy"]
        if not _in(hi - W["cld_coverage"], 2.0 ** -30, 8):
            return False
        mrd = W["max_height"] * F(4.)
        ts = max(mrd / F(W["cloud_steps"]), W["max_height"] / F(W["shadow_steps"]))
        if not _in(np.abs(W["absorb"]) * ts, 0, 80):
            return False
        if not _in(np.abs(W["cloud_light"]), e20, 2.0 ** 20):
            return False
    return rotations_tame(W)


def camera_tame(W):
    """planet_world_camera_tame: the domain of the literal tier's short forms"""
    with np.errstate(all="ignore"):
        if not all(_in(np.abs(c), 0, 256) for c in W["eye"] + W["look_at"]) or not _in(np.abs(W["fov"]), 0, 16):
            return False
        eye, look_at = W["eye"], W["look_at"]
        fwd = normalize((look_at[0] - eye[0], look_at[1] - eye[1], look_at[2] - eye[2]))
        right = (ONE * fwd[2] - fwd[1] * ZERO, ZERO * fwd[0] - fwd[2] * ZERO, ZERO * fwd[1] - fwd[0] * ONE)
        up = (fwd[1] * right[2] - right[1] * fwd[2], fwd[2] * right[0] - right[2] * fwd[0], fwd[0] * right[1] - right[0] * fwd[1])
        if not np.isfinite(np.array(fwd + right + up, dtype=F)).all():
            return False
        ff = sum(float(c) * float(c) for c in fwd)
    return abs(ff - 1.0) <= 1e-5 and rotations_tame(W)


def literal_numbers(W):
    D = default_world(0.)
    return all(_same(W[k], D[k]) if k not in INT_FIELDS + ("reserved",) else tuple(np.atleast_1d(W[k])) == tuple(np.atleast_1d(D[k]))
               for k in FIELDS if k not in LITERAL_FREE)


def tier_of(W, variant=0):
    """what a launch of the block runs, as sbx_debug_planet_world_launches files it: LITERAL (k_planet<true>'s instantiations), RUNTIME
    (k_planet_world<true>) or PLAIN (k_planet<false> / k_planet_world<false>)"""
    if literal_numbers(W):
        return LITERAL if variant != 1 and camera_tame(W) else PLAIN
    return RUNTIME if variant != 1 and tame(W) else PLAIN


def refused(W):
    """why the app refuses the block, or None"""
    if not 1 <= W["terr_steps"] <= 512:
        return "terr_steps"
    if not 1 <= W["cloud_steps"] <= 256:
        return "cloud_steps"
    if not 1 <= W["shadow_steps"] <= 32:
        return "shadow_steps"
    if any(W["reserved"]):
        return "reserved"
    return None


# ---- the header over the world ---------------------------------------------------------------------------------------------------

def sdf_terrain_map(W, pos, octaves=3):               # :175-199
    h0 = fbm([c * F(2.0987) for c in pos], octaves, 2.0244, .454, .454, _noise)
    n0 = smoothstep(F(.35), F(1.), h0)
    off = W["terrain_offset"]
    h1 = fbm([pos[k] * F(1.50987) + off[k] for k in range(3)], octaves, 2.0244, .454, .454, _rnoise)
    n1 = smoothstep(F(.6), F(1.), h1)
    n = n0 + n1
    return length3(pos) - ONE - n * W["max_height"], n / W["max_height"]


def sdf_terrain_normal(W, p):                         # :201-212
    e = F(0.001)

    def d(k, sign):
        dt = [ZERO, ZERO, ZERO]
        dt[k] = e
        q = [p[c] + dt[c] if sign > 0 else p[c] - dt[c] for c in range(3)]
        return sdf_terrain_map(W, q, 7)[0]

    return normalize((d(0, 1) - d(0, -1), d(1, 1) - d(1, -1), d(2, 1) - d(2, -1)))


def setup_lights(W, L, normal):                       # :217-236
    zero = np.zeros_like(normal[0])
    key = fmax(zero, dot(L, normal))
    c_L = W["key_color"]
    diffuse = [ZERO + key * c_L[k] for k in range(3)]
    hemi = clamp(F(.25) + F(.5) * normal[1], ZERO, ONE)
    fill = (F(.4), F(.6), F(.8))
    diffuse = [diffuse[k] + (hemi * fill[k]) * F(.2) for k in range(3)]
    amb = clamp(F(.12) + F(.8) * fmax(zero, dot((-L[0], -L[1], -L[2]), normal)), ZERO, ONE)
    rev = (F(.4), F(.5), F(.6))
    return [diffuse[k] + amb * rev[k] for k in range(3)]


def illuminate(W, pos, rot, h):                       # :238-298 -> [3] arrays
    w_normal = normalize(pos)
    normal = sdf_terrain_normal(W, pos)
    N = dot(normal, w_normal)
    c_water, c_grass, c_beach, c_rock, c_snow = W["c_water"], W["c_grass"], W["c_beach"], W["c_rock"], W["c_snow"]
    l_water, l_shore, l_grass, l_rock = W["l_water"], W["l_shore"], W["l_grass"], W["l_rock"]
    s = smoothstep(F(.4), F(1.), h)
    a = smoothstep(ONE - F(.3) * s, ONE - F(.2) * s, N)
    rock = [mix(c_rock[k], c_snow[k], a) for k in range(3)]
    a = smoothstep(l_grass, l_rock, h)
    grass = [mix(c_grass[k], rock[k], a) for k in range(3)]
    a = smoothstep(l_shore, l_grass, h)
    shoreline = [mix(c_beach[k], grass[k], a) for k in range(3)]
    a = smoothstep(ZERO, l_water, h)
    water = [mix(c_water[k] / TWO, c_water[k], a) for k in range(3)]
    L = mat_vec(rot, W["sun_dir"])                    # :288, the sun as given
    lit = setup_lights(W, L, normal)
    shoreline = [shoreline[k] * lit[k] for k in range(3)]
    lit = setup_lights(W, L, w_normal)
    ocean = [lit[k] * water[k] for k in range(3)]
    a = smoothstep(l_water, l_shore, h)
    return [mix(ocean[k], shoreline[k], a) for k in range(3)]


def clouds_map(W, c, t_step):
    """clouds_map (:102-119) + integrate_volume (:79-100) on the sampler c = dict(pos, height, tr, radiance, alpha), in place"""
    off = W["cloud_offset"]
    dens = fbm([c["pos"][k] * F(3.2343) + off[k] for k in range(3)], 4, 2.0276, .5, .5, _anoise)
    cov, fuzzy = W["cld_coverage"], W["cld_fuzzy"]
    dens = dens * smoothstep(cov, cov + fuzzy, dens)
    dens = dens * P.band(W["band"][0], W["band"][1], W["band"][2], c["height"])
    T_i = _math("exp", -W["absorb"] * dens * t_step)
    c["tr"] = c["tr"] * T_i
    c["radiance"] = c["radiance"] + dens * (_math("exp", c["height"]) / W["cloud_light"]) * c["tr"] * t_step
    c["alpha"] = c["alpha"] + (ONE - T_i) * (ONE - c["alpha"])


def clouds_march(W, origin, rd, max_travel, rot_cloud):          # :121-141 -> (radiance, alpha)
    n = rd[0].size
    steps = W["cloud_steps"]
    mh = W["max_height"]
    t_step = (mh * F(4.)) / F(steps)
    t = np.zeros(n, dtype=F)
    tr, radiance, alpha = np.ones(n, dtype=F), np.zeros(n, dtype=F), np.zeros(n, dtype=F)
    act = np.arange(n)
    for _ in range(steps):
        act = act[~((t[act] > max_travel[act]) | (alpha[act] >= ONE))]
        if act.size == 0:
            break
        o = [origin[k][act] + t[act] * rd[k][act] for k in range(3)]
        pos = mat_vec(rot_cloud, o)
        c = {"pos": pos, "height": (length3(pos) - ONE) / mh, "tr": tr[act], "radiance": radiance[act], "alpha": alpha[act]}
        t[act] = t[act] + t_step
        clouds_map(W, c, t_step)
        tr[act], radiance[act], alpha[act] = c["tr"], c["radiance"], c["alpha"]
    return radiance, alpha


def clouds_shadow_march(W, origin, direction, rot_cloud):        # :143-160 -> alpha
    n = origin[0].size
    steps = W["shadow_steps"]
    mh = W["max_height"]
    t_step = mh / F(steps)
    t = F(0.)
    c = {"tr": np.ones(n, dtype=F), "radiance": np.zeros(n, dtype=F), "alpha": np.zeros(n, dtype=F)}
    for _ in range(steps):
        o = [origin[k] + t * direction[k] for k in range(3)]
        c["pos"] = mat_vec(rot_cloud, o)
        c["height"] = (length3(c["pos"]) - ONE) / mh
        t = t + t_step
        clouds_map(W, c, t_step)
    return c["alpha"]


def render(W, ro, rd, parts=None):
    """render (:303-367) for rays (ro, rd[3][n]; ro one origin or one per ray) -> rgb[n, 3]; parts as planet_builds_model.render's, and
    t_hit (hit.t, no_hit's where the ray missed), t, dfx, dfy as they stand at :344"""
    n = rd[0].size
    with np.errstate(all="ignore"):
        rot, rot_cloud = rotations(W)
        mh = W["max_height"]
        max_ray_dist = mh * F(4.)
        radius = ONE + mh
        rc = (ZERO - ro[0], ZERO - ro[1], ZERO - ro[2])
        radius2 = radius * radius
        tca = dot(rc, rd)
        d2 = dot(rc, rc) - tca * tca
        thc = np.sqrt(radius2 - d2)
        t0 = tca - thc
        t0 = np.where(t0 < ZERO, tca + thc, t0)
        atm = ~(tca < ZERO) & ~(d2 > radius2) & ~(t0 > P.HIT_T)
        rgb = np.zeros((n, 3), dtype=F)
        miss = np.flatnonzero(~atm)
        if miss.size:
            rgb[miss] = np.stack(background([rd[k][miss] for k in range(3)]), axis=1)
        ground = np.zeros(n, dtype=bool)
        t_out, dfx_out, dfy_out = np.zeros(n, dtype=F), np.ones(n, dtype=F), np.full(n, mh, dtype=F)
        alpha_out = np.zeros(n, dtype=F)
        shadow_out = np.ones(n, dtype=F)
        ia = np.flatnonzero(atm)
        if ia.size:
            m = ia.size
            d = [rd[k][ia] for k in range(3)]
            origin = [(ro[k][ia] if np.ndim(ro[k]) else ro[k]) + d[k] * t0[ia] for k in range(3)]
            tt = np.zeros(m, dtype=F)
            dfx, dfy = np.ones(m, dtype=F), np.full(m, mh, dtype=F)
            pos = [np.zeros(m, dtype=F) for _ in range(3)]
            max_cld = np.full(m, max_ray_dist, dtype=F)
            act = np.arange(m)
            for _ in range(W["terr_steps"]):
                act = act[~(tt[act] > max_ray_dist)]
                if act.size == 0:
                    break
                o = [origin[k][act] + tt[act] * d[k][act] for k in range(3)]
                p = mat_vec(rot, o)
                x, y = sdf_terrain_map(W, p)
                for k in range(3):
                    pos[k][act] = p[k]
                dfx[act], dfy[act] = x, y
                hit = x < P.TERR_EPS
                max_cld[act[hit]] = tt[act[hit]]
                go = ~hit
                tt[act[go]] = tt[act[go]] + x[go] * F(.4567)
                act = act[go]
            radiance, alpha = clouds_march(W, origin, d, max_cld, rot_cloud)
            alpha_out[ia] = alpha
            g = dfx < P.TERR_EPS
            ground[ia] = g
            t_out[ia], dfx_out[ia], dfy_out[ia] = tt, dfx, dfy
            ig = np.flatnonzero(g)
            if ig.size:
                ph = [pos[k][ig] for k in range(3)]
                c_terr = illuminate(W, ph, rot, dfy[ig])
                lp = mat_vec(transpose(rot), ph)
                sa = clouds_shadow_march(W, lp, normalize(lp), rot_cloud)
                shadow = mix(F(.7), F(1.), np.where(F(0.33) < sa, ZERO, ONE).astype(F))
                shadow_out[ia[ig]] = shadow
                for k in range(3):
                    rgb[ia[ig], k] = np.abs(mix(c_terr[k] * shadow, radiance[ig], alpha[ig]))
            isky = np.flatnonzero(~g)
            if isky.size:
                bg = background([d[k][isky] for k in range(3)])
                for k in range(3):
                    rgb[ia[isky], k] = np.abs(mix(bg[k], radiance[isky], alpha[isky]))
        if parts is not None:
            parts.update(atm=atm, ground=ground, alpha=alpha_out, shadow=shadow_out, t_hit=np.where(atm, t0, P.HIT_T).astype(F), t=t_out,
                         dfx=dfx_out, dfy=dfy_out)
    return rgb


# ---- sbx_planet_world_eval: tests/planet_eval_model.py's eight functions over a world ---------------------------------------------------

def _cols(v):
    v = _f(v)
    return [np.ascontiguousarray(v[..., k]) for k in range(v.shape[-1])]


def clouds_density(W, x):
    """x [n, 4] (cloud.pos, cloud.height) -> [n, 1]: `dens` of clouds_map :106-114"""
    c = _cols(_f(x).reshape(-1, 4))
    off = W["cloud_offset"]
    with np.errstate(all="ignore"):
        dens = fbm([c[k] * F(3.2343) + off[k] for k in range(3)], 4, 2.0276, .5, .5, _anoise)
        cov, fuzzy = W["cld_coverage"], W["cld_fuzzy"]
        dens = dens * smoothstep(cov, cov + fuzzy, dens)
        dens = dens * P.band(W["band"][0], W["band"][1], W["band"][2], c[3])
    return dens.astype(F).reshape(-1, 1)


def evaluate(W, fn, x):
    """the model of sbx_planet_world_eval(fn, W, x): the layouts of tests/planet_eval_model.py"""
    with np.errstate(all="ignore"):
        if fn in ("render", "terrain_march"):
            c = _cols(_f(x).reshape(-1, 6))
            parts = {}
            rgb = render(W, c[:3], c[3:], parts)
            if fn == "render":
                return np.concatenate([rgb, parts["alpha"][:, None]], axis=1).astype(F)
            return np.stack([parts["t_hit"], parts["t"], parts["dfx"], parts["dfy"]], axis=1).astype(F)
        if fn in ("sdf_terrain_map", "sdf_terrain_map_detail"):
            return np.stack(sdf_terrain_map(W, _cols(_f(x).reshape(-1, 3)), 3 if fn == "sdf_terrain_map" else 7), axis=1).astype(F)
        if fn == "sdf_terrain_normal":
            return np.stack(sdf_terrain_normal(W, _cols(_f(x).reshape(-1, 3))), axis=1).astype(F)
        if fn == "clouds_density":
            return clouds_density(W, x)
        if fn == "illuminate":
            c = _cols(_f(x).reshape(-1, 4))
            return np.stack(illuminate(W, c[:3], rotations(W)[0], c[3]), axis=1).astype(F)
        assert fn == "background", fn
        return np.stack(background(_cols(_f(x).reshape(-1, 3))), axis=1).astype(F)


def main_image(W, width, height, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    with np.errstate(all="ignore"):
        pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), F(W["fov"]))
        rd = get_primary_ray(pcx, pcy, W["eye"], W["look_at"])
        rgb = render(W, _vec(W["eye"]), rd, parts)
        out = np.ones((fx.size, 4), dtype=F)
        out[:, :3] = _math("pow", np.ascontiguousarray(rgb), F(1) / F(2.2))
    return out.reshape(shape + (4,))


def frame(W, width, height, parts=None):
    """float32 [H, W, 4] (row 0 = bottom; fragCoord = pixel centre)"""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(W, width, height, fx, fy, parts)


def points(W, width, height, frag):
    frag = np.asarray(frag, dtype=F).reshape(-1, 2)
    return main_image(W, width, height, frag[:, 0], frag[:, 1])


def fixture_points(seed, w, h, n):
    """the n seeded off-centre fragCoords of a world"""
    return (np.random.default_rng(seed).uniform(0, 1, size=(n, 2)) * [w, h]).astype(F)


def fixture(name):
    """tests/golden/planet_worlds/<name>_WxH.npz (tools/make_golden_planet_worlds.py: the reference's own header with the world written
    into it): block [56] uint32, frame [h, w, 4], points [n, 2], points_out [n, 4]"""
    return np.load(os.path.join(GOLDEN, "planet_worlds", "%s_%dx%d.npz" % (name, SIZE[0], SIZE[1])))


def differing(a, b):
    """the pixels at which two frames differ in a bit"""
    return (~same_bits(a, b)).any(axis=-1)


def classes(parts, shape):
    """-> dict of bool [h, w]: shell (the ray meets the atmosphere), ground, cloud over ground, cloud over sky, bare sky"""
    atm, ground, alpha = (parts[k].reshape(shape) for k in ("atm", "ground", "alpha"))
    cloudy = atm & (alpha > 0)
    return dict(shell=atm, ground=ground, cloud_ground=cloudy & ground, cloud_sky=cloudy & ~ground, sky=~atm)


# What the REFERENCE's 64x36 frames show (pixels of 2304; tools/make_golden_planet_worlds.py prints them), and beside them the floors
# of check_conditions, about half of each.  The default world at u_time .37: shell 1304, ground 672, cloud over ground 502, cloud over
# sky 352, sky 1000, 25 NaN pixels.
#   orbit       shell  794  ground 385  cloud/ground 308  cloud/sky 201  sky 1510   792 shell pixels differ from the default's, 34 NaN
#   recoloured        1304         672               502            352       1000   647, 25 NaN
#   overcast          1304         672               648            476       1000  1117, 25 NaN
#   alpine            1600         712               587            482        704  1182, 33 NaN
#   landing           1640         625               369            351        664  1640,  2 NaN
FLOORS = {
    "orbit": dict(shell=400, ground=190, cloud_ground=150, cloud_sky=100, sky=750),
    "recoloured": dict(shell=650, ground=335, cloud_ground=250, cloud_sky=175, sky=500),
    "overcast": dict(shell=650, ground=335, cloud_ground=325, cloud_sky=240, sky=500),
    "alpine": dict(shell=800, ground=355, cloud_ground=290, cloud_sky=240, sky=350),
    "landing": dict(shell=820, ground=310, cloud_ground=185, cloud_sky=175, sky=330),
}


def check_conditions(frames, parts_of, default_frame):
    """The conditions under which the fixture worlds say something, over {name: frame}, {name: parts} and the default world's frame of
    u_time T0.  Conditions, not measurements."""
    assert set(frames) == set(WORLDS) == set(parts_of)
    for name, f in frames.items():
        c = classes(parts_of[name], f.shape[:2])
        for k, floor in FLOORS[name].items():
            assert c[k].sum() >= floor, (name, k, int(c[k].sum()), floor)
        d = differing(f, default_frame) & c["shell"]
        assert d.sum() >= .25 * c["shell"].sum(), (name, "differs from the default world's frame", int(d.sum()), int(c["shell"].sum()))
        assert (f[..., 3] == 1).all()
    assert tier_of(WORLDS["orbit"]) == LITERAL
    for name in ("recoloured", "overcast", "alpine", "landing"):
        assert tier_of(WORLDS[name]) == RUNTIME and tame(WORLDS[name]), name


def single_field_worlds():
    """{field: world}: default_world(T0) with that field alone changed"""
    other = dict(eye=(.2, .1, -2.4), fov=.5, look_at=(.1, .1, 2.), tilt_deg=20., sun_dir=(0., 1., 0.), spin_deg=30., key_color=(5, 5, 5),
                 cloud_spin_deg=-15., terrain_offset=(2., 2.435, .5483), max_height=.45, cloud_offset=(.35, 13.5, 2.67), cld_coverage=.31,
                 band=(.2, .4, .65), cld_fuzzy=.05, c_water=(.015, .2, .455), l_water=.06, c_grass=(.1, .132, .018), l_shore=.18,
                 c_beach=(.2, .172, .121), l_grass=.25, c_rock=(.1, .05, .03), l_rock=.4, c_snow=(.7, .6, .6), absorb=20., cloud_light=.07,
                 terr_steps=40, cloud_steps=60, shadow_steps=3)
    assert set(other) == set(FIELDS) - {"reserved"}
    return {k: world(T0, **{k: v}) for k, v in other.items()}
