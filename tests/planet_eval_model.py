"""numpy restatement of sbx_planet_eval (include/sbx.h): the eight functions of src/app_planet.h as shipped over the caller's elements,
in binary32, built on tests/planet_builds_model.py — whose sdf_terrain_map, sdf_terrain_normal, illuminate, clouds_march,
clouds_shadow_march, background, smoothstep, band and fbm are imported as they stand — plus render (:303-367) with a per-element ray
origin, the terrain march on its own and the density of clouds_map.  tests/test_planet_eval_cpu.py pins the module to the oracle's
frames and hooks and to the frame the reference's own header rendered from the close-up eye; the input families that the CPU and GPU
tests share are stated here too.
"""
import numpy as np

from tests import planet_builds_model as PB
from tests.egg_builds_model import mat_vec, mix
from tests.model_common import F, ONE, ZERO, _f, dot, get_primary_ray, normalize, point_cam
from tests.vinyl_builds_model import mat_mat, rotate_around_x, rotate_around_y

WIDTHS = {"render": (6, 4), "terrain_march": (6, 4), "sdf_terrain_map": (3, 2), "sdf_terrain_map_detail": (3, 2),
          "sdf_terrain_normal": (3, 3), "clouds_density": (4, 1), "illuminate": (4, 3), "background": (3, 3)}
FNS = tuple(WIDTHS)
TIME_FNS = ("render", "terrain_march", "illuminate")        # the three that read u_time
GUARDED_FNS = tuple(f for f in FNS if f != "background")    # the functions with guarded short forms
TIMES = (0.0, 0.37)
EYES = {"shipped": PB.CAMERA["default"], "closeup": PB.CAMERA["closeup"]}


def _cols(v):
    v = _f(v)
    return [np.ascontiguousarray(v[..., k]) for k in range(v.shape[-1])]


def linear_to_srgb(rgb):                            # util.h:72-77 as mainImage applies it
    rgb = np.ascontiguousarray(_f(rgb))
    return PB._math("pow", rgb, F(1) / F(2.2))


def rotations(u_time):                              # :307-309
    t = F(u_time)
    rot_y = rotate_around_y(27.)
    return mat_mat(rotate_around_x(t * F(-12.)), rot_y), mat_mat(rotate_around_x(t * F(8.)), rot_y)


def trace(rays, u_time=0.0, clouds=True):
    """render (:303-367) over rays [n, 6] with a per-element origin -> a dict: rgb [n, 3]; alpha (cloud.alpha as read at :352 / :365,
    0 where :320 returned); atm; t_hit (hit.t, no_hit's where the ray missed); t, dfx, dfy as they stand at :344; ground (:349);
    shadow (the value at :363, 1 elsewhere); hit_o [n, 3].  clouds=False stops after the terrain march (rgb, alpha, shadow unset)."""
    c = _cols(_f(rays).reshape(-1, 6))
    ro, rd = c[:3], c[3:]
    n = rd[0].size
    with np.errstate(all="ignore"):
        rot, rot_cloud = rotations(u_time)
        # intersect_sphere(eye, {planet.origin, 1 + max_height}, no_hit)   intersect.h:7-33
        radius = ONE + PB.MAX_HEIGHT
        rc = (ZERO - ro[0], ZERO - ro[1], ZERO - ro[2])
        radius2 = radius * radius
        tca = dot(rc, rd)
        d2 = dot(rc, rc) - tca * tca
        thc = np.sqrt(radius2 - d2)
        t0 = tca - thc
        t0 = np.where(t0 < ZERO, tca + thc, t0)
        atm = ~(tca < ZERO) & ~(d2 > radius2) & ~(t0 > PB.HIT_T)
        out = {"atm": atm, "t_hit": np.where(atm, t0, PB.HIT_T).astype(F), "t": np.zeros(n, dtype=F), "dfx": np.ones(n, dtype=F),
               "dfy": np.full(n, PB.MAX_HEIGHT, dtype=F), "ground": np.zeros(n, dtype=bool), "alpha": np.zeros(n, dtype=F),
               "shadow": np.ones(n, dtype=F), "rgb": np.zeros((n, 3), dtype=F), "hit_o": np.zeros((n, 3), dtype=F)}
        miss = np.flatnonzero(~atm)
        if miss.size and clouds:
            out["rgb"][miss] = np.stack(PB.background([rd[k][miss] for k in range(3)]), axis=1)
        ia = np.flatnonzero(atm)
        if not ia.size:
            return out
        m = ia.size
        d = [rd[k][ia] for k in range(3)]
        origin = [ro[k][ia] + d[k] * t0[ia] for k in range(3)]
        out["hit_o"][ia] = np.stack(origin, axis=1)
        # terrain march :323-342
        tt = np.zeros(m, dtype=F)
        dfx, dfy = np.ones(m, dtype=F), np.full(m, PB.MAX_HEIGHT, dtype=F)
        pos = [np.zeros(m, dtype=F) for _ in range(3)]
        max_cld = np.full(m, PB.MAX_RAY_DIST, dtype=F)
        act = np.arange(m)
        for _ in range(PB.TERR_STEPS):
            act = act[~(tt[act] > PB.MAX_RAY_DIST)]
            if act.size == 0:
                break
            o = [origin[k][act] + tt[act] * d[k][act] for k in range(3)]
            p = mat_vec(rot, o)
            x, y = PB.sdf_terrain_map(p)
            for k in range(3):
                pos[k][act] = p[k]
            dfx[act], dfy[act] = x, y
            hit = x < PB.TERR_EPS
            max_cld[act[hit]] = tt[act[hit]]
            go = ~hit
            tt[act[go]] = tt[act[go]] + x[go] * F(.4567)
            act = act[go]
        g = dfx < PB.TERR_EPS                       # :349
        out["t"][ia], out["dfx"][ia], out["dfy"][ia], out["ground"][ia] = tt, dfx, dfy, g
        if not clouds:
            return out
        radiance, alpha = PB.clouds_march(origin, d, max_cld, rot_cloud)      # :344-347
        out["alpha"][ia] = alpha
        ig = np.flatnonzero(g)
        if ig.size:
            ph = [pos[k][ig] for k in range(3)]
            c_terr = PB.illuminate("default", ph, rot, dfy[ig])
            lp = mat_vec(PB.transpose(rot), ph)     # :355-361
            sa = PB.clouds_shadow_march(lp, normalize(lp), rot_cloud)
            shadow = mix(F(.7), F(1.), np.where(F(0.33) < sa, ZERO, ONE).astype(F))
            out["shadow"][ia[ig]] = shadow
            for k in range(3):
                out["rgb"][ia[ig], k] = np.abs(mix(c_terr[k] * shadow, radiance[ig], alpha[ig]))
        isky = np.flatnonzero(~g)
        if isky.size:                               # :364-366
            bg = PB.background([d[k][isky] for k in range(3)])
            for k in range(3):
                out["rgb"][ia[isky], k] = np.abs(mix(bg[k], radiance[isky], alpha[isky]))
    return out


def render(rays, u_time=0.0):
    """rays [n, 6] -> [n, 4]: the linear RGB of :303-367, then cloud.alpha (0 where :320 returned the background)"""
    tr = trace(rays, u_time)
    return np.concatenate([tr["rgb"], tr["alpha"][:, None]], axis=1).astype(F)


def terrain_march(rays, u_time=0.0):
    """rays [n, 6] -> [n, 4]: hit.t, then t, df.x, df.y at :344"""
    tr = trace(rays, u_time, clouds=False)
    return np.stack([tr["t_hit"], tr["t"], tr["dfx"], tr["dfy"]], axis=1).astype(F)


def sdf_terrain_map(points, octaves=3):
    with np.errstate(all="ignore"):
        return np.stack(PB.sdf_terrain_map(_cols(_f(points).reshape(-1, 3)), octaves), axis=1).astype(F)


def sdf_terrain_map_detail(points):
    return sdf_terrain_map(points, 7)


def sdf_terrain_normal(points):
    with np.errstate(all="ignore"):
        return np.stack(PB.sdf_terrain_normal(_cols(_f(points).reshape(-1, 3))), axis=1).astype(F)


def clouds_density(x):
    """x [n, 4] (cloud.pos, cloud.height) -> [n, 1]: `dens` of clouds_map :106-114"""
    c = _cols(_f(x).reshape(-1, 4))
    off = (F(.35), F(13.35), F(2.67))
    with np.errstate(all="ignore"):
        dens = PB.fbm([c[k] * F(3.2343) + off[k] for k in range(3)], 4, 2.0276, .5, .5, PB._anoise)
        cov, fuzzy = F(.29475675), F(.0335)
        dens = dens * PB.smoothstep(cov, cov + fuzzy, dens)
        dens = dens * PB.band(F(.2), F(.35), F(.65), c[3])
    return dens.astype(F).reshape(-1, 1)


def illuminate(x, u_time=0.0):
    """x [n, 4] (pos, df.y) -> [n, 3]: illuminate :238-298 with local_xform = rot of u_time"""
    c = _cols(_f(x).reshape(-1, 4))
    with np.errstate(all="ignore"):
        return np.stack(PB.illuminate("default", c[:3], rotations(u_time)[0], c[3]), axis=1).astype(F)


def background(dirs):
    with np.errstate(all="ignore"):
        return np.stack(PB.background(_cols(_f(dirs).reshape(-1, 3))), axis=1).astype(F)


def evaluate(fn, x, u_time=0.0):
    """the model of sbx_planet_eval(fn, u_time, x)"""
    if fn in TIME_FNS:
        return {"render": render, "terrain_march": terrain_march, "illuminate": illuminate}[fn](x, u_time)
    return {"sdf_terrain_map": sdf_terrain_map, "sdf_terrain_map_detail": sdf_terrain_map_detail, "sdf_terrain_normal": sdf_terrain_normal,
            "clouds_density": clouds_density, "background": background}[fn](x)


# ---- the input families (deterministic) ------------------------------------------------------------------------------------------------

def primary_rays(w, h, eye, look_at):
    """the primary rays of main.h's pipeline for a w x h frame (FOV tan(radians(30)), row 0 = bottom, x fastest) -> [w * h, 6]"""
    fx = np.tile(np.arange(w, dtype=F) + F(.5), h)
    fy = np.repeat(np.arange(h, dtype=F) + F(.5), w)
    pcx, pcy = point_cam(w, h, fx, fy, PB.fov())
    d = get_primary_ray(pcx, pcy, eye, look_at)
    return np.concatenate([np.tile(np.array(eye, dtype=F), (w * h, 1)), np.stack(d, axis=-1)], axis=1).astype(F)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def family_a():
    """the primary rays of a 48x27 frame from the shipped eye"""
    return primary_rays(48, 27, *EYES["shipped"])


def family_b():
    """the primary rays of a 24x14 frame from the closeup eye"""
    return primary_rays(24, 14, *EYES["closeup"])


def family_c(seed=11):
    """96 rays whose origins lie inside the shell (|o| in 1.05 .. 1.38), on the ground looking up (|o| = 1.0 .. 1.04 along the local up,
    tilted a little) and below the surface (|o| in .2 .. .95), 32 of each, with unit directions"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(96):
        u = _unit(rng.normal(size=3))
        kind = k // 32
        if kind == 0:
            o, d = u * rng.uniform(1.05, 1.38), _unit(rng.normal(size=3))
        elif kind == 1:
            o, d = u * rng.uniform(1.0, 1.04), _unit(u + .3 * rng.normal(size=3))
        else:
            o, d = u * rng.uniform(.2, .95), _unit(rng.normal(size=3))
        rows.append([*o, *d])
    return np.array(rows, dtype=F)


def family_d(seed=12):
    """64 far rays: 40 from 10^3 away aimed at a point within .9 of the centre (they meet the planet), 12 with coordinates of 10^6 and
    12 of 10^9 aimed at the centre"""
    rng = np.random.default_rng(seed)
    rows = []
    for k in range(64):
        u = _unit(rng.normal(size=3))
        dist = 1e3 if k < 40 else 1e6 if k < 52 else 1e9
        o = u * dist
        aim = rng.uniform(-.5, .5, size=3) if k < 40 else np.zeros(3)
        rows.append([*o, *_unit(aim - o)])
    return np.array(rows, dtype=F)


def family_e():
    """the specials"""
    nan, inf = float("nan"), float("inf")
    u = _unit([.3, .6, -.2])
    eye = (0.0, 0.0, -2.5)
    fwd = (0.0, 0.0, 1.0)
    rows = [[0, 0, -2.5, 0, 0, 0],                                      # a zero direction from outside: no shell hit but tca = 0
            [0, 0, 0, 0, 0, 0],                                         # ... from the exact centre: a ground hit at pos = 0, normalize 0/0
            [0, 0, 0, *u],                                              # the exact centre, looking out
            [.5, 0, 0, 0, 0, 0],                                        # a zero direction from below the surface
            [0, 0, -2.5, *fwd],                                         # the centre ray: a hit point with two zero coordinates before rot
            [0, 1.2, 0, 0, -1, 0],                                      # a zero coordinate pair in the origin, straight down
            [0, 0, -2.5, *(2.0 * np.array(fwd))],                       # directions of length 2 and .5
            [0, 0, -2.5, *(.5 * np.array(fwd))],
            [.3, .2, -2.5, *(2.0 * _unit([-.1, -.05, 1]))],
            [.3, .2, -2.5, *(.5 * _unit([-.1, -.05, 1]))],
            [1e-40, -1e-40, -2.5, 1e-41, 0, 1],                         # denormals
            [0, 0, -2.5, 1e-39, -1e-42, 1e-38],
            [1e-39, 1e-39, 1e-39, *u],
            [3e38, 0, -3e38, *u],                                       # the largest finite origins
            [0, 0, -2.5, 1e30, 1e30, 1e30]]                             # a huge direction
    for slot in range(6):                                               # NaN, +inf, -inf in each slot
        for v in (nan, inf, -inf):
            r = [*eye, *fwd] if slot >= 3 else [.2, .1, -2.5, *fwd]
            r[slot] = v
            rows.append(r)
    return np.array(rows, dtype=np.float64).astype(F)


_FAMILIES = {}


def family(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}[name]()
    return _FAMILIES[name]


def rays(names="abcde"):
    """the families concatenated -> float32 [n, 6]"""
    return np.concatenate([family(n) for n in names], axis=0)


def _stride(x, count):
    """about `count` rows of x, evenly spread"""
    return x[::max(1, len(x) // count)]


def points(names="abcde"):
    """the point set of the families: where a ray meets the shell and where its terrain march ended, rotated as the march rotates them
    (both times), for a spread of the rays of A-C; for D the rays' origins and -.75 times them (coordinates of 10^3, 10^6, 10^9: lattice
    indices beyond 2^22); for E the rays' origins and directions as they stand (NaN, inf, zeros, denormals) and six points with zero
    coordinates"""
    out = []
    for nm in names:
        r = family(nm)
        if nm in "abc":
            r = _stride(r, 40)
            for t in TIMES:
                tr = trace(r, t, clouds=False)
                k = np.flatnonzero(tr["atm"])
                with np.errstate(all="ignore"):
                    rot = rotations(t)[0]
                    for tt in (np.zeros(k.size, dtype=F), tr["t"][k]):
                        o = [tr["hit_o"][k, c] + tt * r[k, 3 + c] for c in range(3)]
                        out.append(np.stack(mat_vec(rot, o), axis=1))
        elif nm == "d":
            out += [r[:, :3], r[:, :3] * F(-.75)]
        else:
            out += [r[:, :3], r[:, 3:]]
            if nm == "e":
                out.append(np.array([[0, .7, .8], [.9, 0, .5], [.6, .9, 0], [-0.0, 1.05, .1], [1, 0, 0], [0, 0, 0]], dtype=F))   # zero coordinates: the unpaired normal
    return np.concatenate(out, axis=0).astype(F)


def inputs(fn, names="abcde"):
    """what the tests feed `fn`: the rays, their directions, the point set, or the point set with a fourth column (clouds_density: a
    height that sweeps the band and its outside, the specials' own values at the end; illuminate: df.y sweeping 0 .. 2.5)"""
    if fn in ("render", "terrain_march"):
        return rays(names)
    if fn == "background":
        return np.ascontiguousarray(rays(names)[:, 3:])
    p = points(names)
    if fn in ("clouds_density", "illuminate"):
        k = np.arange(len(p))
        w = (F(-.3) + F(1.4) * ((k % 29) / F(28))) if fn == "clouds_density" else F(2.5) * ((k % 23) / F(22))
        w = np.asarray(w, dtype=F)
        if "e" in names:
            w[-6:] = np.array([np.nan, np.inf, -np.inf, 1e35, 0.0, -1e-40], dtype=F)
        return np.concatenate([p, w[:, None]], axis=1).astype(F)
    return p
