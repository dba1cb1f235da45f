"""numpy restatement of sbx_clouds_eval (include/sbx.h): the five functions of src/app_clouds.h's procedural build over the caller's
elements, in binary32, built on tests/clouds_builds_model.py — whose render_clouds, render_sky_color, density_func and light_march
take a per-ray eye as they stand — plus render (:204-218) without its camera and illuminate_volume (:91-123) with its phase function.
tests/test_clouds_eval_cpu.py pins the module to the oracle's frames and hooks bit for bit; the input families, point sets and aux
sets that the CPU and GPU tests share are stated here too.
"""
import numpy as np

from tests import clouds_builds_model as CB
from tests.model_common import F, ONE, TWO, ZERO, _f, dot, get_primary_ray, point_cam

WIDTHS = {"render": (6, 4), "render_clouds": (6, 4), "render_sky_color": (3, 3), "density_func": (3, 1), "illuminate_volume": (6, 1)}
FNS = tuple(WIDTHS)
TIMES = (0.0, 1.5)
EYE = (0.0, -.5, 0.0)                               # setup_camera :23-30
MOUSES = ((0.0, 0.0), (1.3, 0.0))


def _general_sun():
    s = (F(.3), F(.5), F(-.8))
    n = np.sqrt(dot(s, s))
    return tuple(float(c / n) for c in s)           # normalised in binary32


# the aux sets, as the fields that differ from the defaults (every value a binary32 number)
AUX = {
    "default": None,
    "general_sun": {"sun_dir": _general_sun(), "wind_dir": tuple(float(F(v)) for v in (.1, .05, .2)), "cld_coverage": float(F(.6))},
    "exp_outside": {"cld_march_steps": 37, "illum_march_steps": 3, "sigma_scattering": 2.0, "cld_thick": 400.0},   # beyond exp_small_
    "cov_one": {"cld_coverage": 1.0},               # cov = 0 fails clouds_div3_domain
}


def _cols(v):
    v = _f(v)
    return [np.ascontiguousarray(v[..., k]) for k in range(v.shape[-1])]


def linear_to_srgb(rgb):                            # util.h:72-77 as main_image applies it
    rgb = _f(rgb)
    return CB._pow(rgb.ravel(), F(1) / F(2.2)).reshape(rgb.shape)


def render_sky_color(dirs, aux=None):
    """dirs [n, 3] -> [n, 3]"""
    A = CB.aux_block(aux)
    with np.errstate(all="ignore"):
        return np.stack(CB.render_sky_color(_cols(_f(dirs).reshape(-1, 3)), A), axis=-1).astype(F)


def density_func(points, aux=None):
    """points [n, 3] -> [n, 1]"""
    A = CB.aux_block(aux)
    with np.errstate(all="ignore"):
        return CB.density_func(_cols(_f(points).reshape(-1, 3)), A).astype(F).reshape(-1, 1)


def illuminate_volume(x, aux=None):
    """x [n, 6] (origin, V) -> [n, 1]: light_march * sun_power * henyey_greenstein(clamp(dot(L, V), 0, 1)) with L = sun_dir, :121"""
    A = CB.aux_block(aux)
    c = _cols(_f(x).reshape(-1, 6))
    with np.errstate(all="ignore"):
        dt = A["cld_thick"] / F(int(A["cld_march_steps"]))
        lum = CB.light_march(c[:3], A, dt)
        mu = CB.clamp(dot(A["sun_dir"], c[3:]), ZERO, ONE)
        phase = (ONE - CB.HG_G * CB.HG_G) / ((F(4.) + CB.PI) * CB._pow(ONE + CB.HG_G * CB.HG_G - TWO * CB.HG_G * mu, 1.5))
        return ((lum * A["sun_power"]) * phase).astype(F).reshape(-1, 1)


def render_clouds(rays, u_time=0.0, aux=None):
    """rays [n, 6] -> [n, 4]: the vec4 of :201"""
    A = CB.aux_block(aux)
    c = _cols(_f(rays).reshape(-1, 6))
    rad, a = CB.render_clouds("default", c[3:], c[:3], u_time, A)
    return np.stack([rad, rad, rad, a], axis=-1).astype(F)


def render(rays, u_time=0.0, aux=None):
    """rays [n, 6] -> [n, 4]: the linear RGB of :204-218, then the alpha render_clouds returned (0 where :212 returned the sky)"""
    A = CB.aux_block(aux)
    rays = _f(rays).reshape(-1, 6)
    c = _cols(rays)
    d = c[3:]
    with np.errstate(all="ignore"):
        sky = CB.render_sky_color(d, A)
        out = np.zeros((len(rays), 4), dtype=F)
        for k in range(3):
            out[:, k] = sky[k]
        m = np.nonzero(~(dot(d, (ZERO, ONE, ZERO)) < F(0.05)))[0]
        if m.size:
            cl = render_clouds(rays[m], u_time, aux)
            for k in range(3):
                out[m, k] = np.abs(CB.mix(sky[k][m], cl[:, 0], cl[:, 3]))
            out[m, 3] = cl[:, 3]
    return out


MODEL = {"render": render, "render_clouds": render_clouds}


def evaluate(fn, x, u_time=0.0, aux=None):
    """the model of sbx_clouds_eval(fn, aux, u_time, x)"""
    if fn in MODEL:
        return MODEL[fn](x, u_time, aux)
    return {"render_sky_color": render_sky_color, "density_func": density_func, "illuminate_volume": illuminate_volume}[fn](x, aux)


# ---- the input families (deterministic) ------------------------------------------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def primary_rays(w, h, mouse=(0.0, 0.0)):
    """the primary rays of a w x h APP_CLOUDS frame, row 0 = bottom, x fastest -> [w * h, 6]"""
    fx = np.tile(np.arange(w, dtype=F) + F(.5), h)
    fy = np.repeat(np.arange(h, dtype=F) + F(.5), w)
    pcx, pcy = point_cam(w, h, fx, fy, CB.FOV)
    eye, look_at = CB.setup_camera(mouse)
    d = get_primary_ray(pcx, pcy, eye, look_at)
    return np.concatenate([np.tile(np.array(EYE, dtype=F), (w * h, 1)), np.stack(d, axis=-1)], axis=1).astype(F)


def family_a():
    """the primary rays of a 16x9 frame at mouse (0, 0) and (1.3, 0)"""
    return np.concatenate([primary_rays(16, 9, m) for m in MOUSES], axis=0)


def _up_dirs(rng, n):
    """unit directions with dir.y >= .1"""
    out = []
    while len(out) < n:
        d = _unit(rng.normal(size=3))
        if d[1] >= .1:
            out.append(d)
    return np.array(out)


def family_b(seed=5):
    """40 rays with origins uniform in +-2000 per axis and unit directions with dir.y >= .1"""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-2000, 2000, size=(40, 3))
    return np.concatenate([o, _up_dirs(rng, 40)], axis=1).astype(F)


def family_c(seed=6):
    """20 rays at and under the horizon cut of :212: dir.y on both binary32 neighbours of 0.05 and on 0.05 itself, exactly 0, -0, and
    negative; the horizontal part has the length that makes the direction a unit vector"""
    rng = np.random.default_rng(seed)
    cut = F(0.05)
    ys = [np.nextafter(cut, F(0)), np.nextafter(cut, F(1)), cut, F(0.0), F(-0.0), F(-.3), F(.049), F(-1e-3), F(.02), F(-.9)]
    rows = []
    for i in range(20):
        y = ys[i % len(ys)]
        phi = rng.uniform(0, 2 * np.pi)
        r = np.sqrt(1.0 - float(y) ** 2)
        o = rng.uniform(-500, 500, size=3)
        rows.append([F(o[0]), F(o[1]), F(o[2]), F(r * np.cos(phi)), y, F(r * np.sin(phi))])
    return np.array(rows, dtype=F)


def lattice_indices(points):
    """noise_iq's n = px + py * 157 + 113 * pz of density_func's four octaves at points [n, 3] -> [n, 4], in binary32"""
    p = [(c * CB.NOISE_FACTOR) * F(2.03) for c in _cols(_f(points).reshape(-1, 3))]
    out = []
    with np.errstate(all="ignore"):
        for _ in range(4):
            fl = [np.floor(c) for c in p]
            out.append((fl[0] + fl[1] * F(157.0)) + F(113.0) * fl[2])
            p = [c * F(2.64) for c in p]
    return np.stack(out, axis=-1)


def march_points(rays, u_time=0.0, aux=None, steps=(0, 50, 99)):
    """positions render_clouds samples along rays [n, 6] at the given main steps (t = step * dt in binary64, rounded: for range
    checks, not for bits) -> [n * len(steps), 3]"""
    A = CB.aux_block(aux)
    c = _cols(_f(rays).reshape(-1, 6))
    with np.errstate(all="ignore"):
        proj = [c[3 + k] / c[4] for k in range(3)]
        wind = [(A["wind_dir"][k] * F(u_time)) * (ONE / CB.NOISE_FACTOR) for k in range(3)]
        origin = [(c[k] + proj[k] * F(150.)) + wind[k] for k in range(3)]
        dt = A["cld_thick"] / F(int(A["cld_march_steps"]))
        return np.concatenate([np.stack([origin[k] + F(s * float(dt)) * proj[k] for k in range(3)], axis=-1) for s in steps], axis=0)


def family_d(seed=7):
    """40 far rays with B's directions: origins in +-2e5 per axis for the first 20; for the other 20 every coordinate between 1e8 and
    3e8 in magnitude, drawn until no lattice index along the ray's march or at its origin (in any octave) lies within 2^22"""
    rng = np.random.default_rng(seed)
    dirs = family_b()[:, 3:]
    near = np.concatenate([rng.uniform(-2e5, 2e5, size=(20, 3)), dirs[:20]], axis=1).astype(F)
    far = []
    while len(far) < 20:
        o = rng.uniform(1e8, 3e8, size=3) * rng.choice([-1.0, 1.0], size=3)
        ray = np.concatenate([o, dirs[20 + len(far)]]).astype(F)
        pts = np.concatenate([march_points(ray[None], t) for t in TIMES] + [ray[None, :3]], axis=0)      # (the origin: illuminate_volume's)
        pts = np.concatenate([pts, pts + F(800), pts - F(800)], axis=0)      # a light march reaches a few units, far less than the ulp here
        if (np.abs(lattice_indices(pts)) > F(2.0 ** 22) + F(271)).all():
            far.append(ray)
    return np.concatenate([near, np.array(far, dtype=F)], axis=0)


def family_e():
    """the specials"""
    nan, inf = float("nan"), float("inf")
    u = _unit([.3, .6, -.2])
    rows = [
        [nan, 0, 0, *u],                                                    # NaN in the origin
        [0, -.5, 0, nan, .6, .8],                                           # NaN in the direction
        [0, -.5, 0, .6, nan, .8],                                           # ... in dir.y
        [inf, 0, 0, *u],                                                    # inf in the origin
        [0, -inf, 0, *u],
        [0, -.5, 0, inf, .6, .8],                                           # inf in the direction
        [0, -.5, 0, .6, inf, .8],
        [0, -.5, 0, 0, 0, 0],                                               # the zero direction
        [10, 20, 30, *(2.0 * u)],                                           # non-unit directions
        [10, 20, 30, *(.25 * u)],
        [0, -.5, 0, .6, 1e-40, .8],                                         # a subnormal dir.y
        [0, -.5, 0, .6, -1e-40, .8],
        [0, -.5, 0, 0, 1, 0],                                               # straight up
        [3e38, 0, -3e38, *u],                                               # the largest finite origins
        [0, -.5, 0, 1e30, 1e30, -1e30],                                     # a huge direction
    ]
    return np.array(rows, dtype=np.float64).astype(F)


_FAMILIES = {}


def family(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = {"a": family_a, "b": family_b, "c": family_c, "d": family_d, "e": family_e}[name]()
    return _FAMILIES[name]


def rays(names="abcde"):
    """the families concatenated -> float32 [n, 6]"""
    return np.concatenate([family(n) for n in names], axis=0)


def points(names="bcde", seed=8):
    """density_func's point set: the position every ray of the families first samples at both times, plus 24 points scaled to +-3e9"""
    rng = np.random.default_rng(seed)
    r = rays(names)
    first = [march_points(r, t, steps=(0,)) for t in TIMES]
    big = rng.uniform(-1, 1, size=(24, 3)) * 3e9
    return np.concatenate(first + [big], axis=0).astype(F)


def inputs(fn, names="abcde"):
    """what the tests feed `fn`: the rays, their directions, or the point set"""
    if fn == "render_sky_color":
        return np.ascontiguousarray(rays(names)[:, 3:])
    if fn == "density_func":
        return points(names)
    return rays(names)
