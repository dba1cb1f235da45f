"""numpy restatement of sbx_atmosphere_eval (include/sbx.h): get_incident_light and get_sun_light of src/app_atmosphere.h:50-160 over
arbitrary rays with an EXPLICIT sun direction, which the oracle's hooks (`atmosphere.get_incident_light`, `atmosphere.get_sun_light`)
cannot take: they rotate (0, 1, 0) by u_time.  Binary32 step by step in the oracle's operation order (oracle/ovec.h: dot =
(x x + y y) + z z, length = sqrt of it; oracle/ref_apps.h:523-580: march_pos + .5f * march_step, IEEE divisions by hR, hM, 8 and
16), exp and pow through the oracle's own (`oracle().math`), all rays at once.  get_sun_light's early return is a per-ray mask that
freezes the sums.  tests/test_atmosphere_eval_cpu.py pins the module to both hooks bit for bit; the ray families the CPU and GPU
tests share are stated here too.
"""
import numpy as np

from tests.model_common import F, ZERO, ONE, _f, dot, oracle

EARTH_RADIUS = F(6360e3)                            # src/app_atmosphere.h:37
ATMOSPHERE_RADIUS = F(6420e3)                       # :38
HR, HM = F(7994.0), F(1200.0)                       # :34-35
BETA_R = (F(5.5e-6), F(13.0e-6), F(22.4e-6))        # :29
BETA_M = (F(21e-6), F(21e-6), F(21e-6))             # :30
SUN_POWER = F(20.0)                                 # :41
HG_G = F(.76)                                       # :12
PI = F(3.14159265359)
TIMES = (0.0, .37, 2.0, 3.1, 100.25)
# suns the u_time hook cannot make (the GPU tests' second reference is this module)
SUNS = ((.6, .48, -.64), (0.0, -1.0, 0.0), (1e-3, 1e-3, 1.0), (0.0, 2.0, 0.0), (0.0, 0.0, 0.0), (float("nan"), 1.0, 0.0))


def _exp(x):
    x = _f(x)
    return oracle().math("exp", x.ravel()).reshape(x.shape)


def _cols(v):
    """[n, 3] (or a 3-tuple) -> three float32 arrays"""
    if isinstance(v, tuple):
        return tuple(_f(c) for c in v)
    v = _f(v)
    return v[..., 0], v[..., 1], v[..., 2]


def isect_atmosphere(ro, rd):                       # oracle/ref_apps.h:523-532 with sphere (0, atmosphere_radius)
    rc = (ZERO - ro[0], ZERO - ro[1], ZERO - ro[2])
    radius2 = ATMOSPHERE_RADIUS * ATMOSPHERE_RADIUS
    tca = dot(rc, rd)
    d2 = dot(rc, rc) - tca * tca
    thc = np.sqrt(radius2 - d2)
    return d2 < radius2, tca + thc, d2


def _sample(ro, rd, t):
    return (ro[0] + rd[0] * t, ro[1] + rd[1] * t, ro[2] + rd[2] * t)


def _sun_light(ro, rd):
    """-> (overground, optical_depthR, optical_depthM), the depths starting at 0 and frozen where the march returned"""
    with np.errstate(all="ignore"):
        _, t1, _ = isect_atmosphere(ro, rd)
        odr = np.zeros(t1.shape, dtype=F)
        odm = np.zeros(t1.shape, dtype=F)
        alive = np.ones(t1.shape, dtype=bool)
        march_pos = np.zeros(t1.shape, dtype=F)
        march_step = t1 / F(8)
        for _ in range(8):
            s = _sample(ro, rd, march_pos + F(.5) * march_step)
            height = np.sqrt(dot(s, s)) - EARTH_RADIUS
            alive = alive & ~(height < ZERO)
            odr = np.where(alive, odr + _exp(-height / HR) * march_step, odr)
            odm = np.where(alive, odm + _exp(-height / HM) * march_step, odm)
            march_pos = march_pos + march_step
        return alive, odr, odm


def get_sun_light(rays):
    """rays [n, 6] -> float32 [n, 3] = (overground ? 1 : 0, optical_depthR, optical_depthM)"""
    rays = _f(rays).reshape(-1, 6)
    ro, rd = _cols(rays[:, :3]), _cols(rays[:, 3:])
    ok, odr, odm = _sun_light(ro, rd)
    return np.stack([np.where(ok, ONE, ZERO), odr, odm], axis=-1).astype(F)


def get_incident_light(rays, sun_dir):
    """rays [n, 6], sun_dir 3 values (used as given) -> float32 [n, 3], the linear RGB of :78-160"""
    rays = _f(rays).reshape(-1, 6)
    n = len(rays)
    ro, rd = _cols(rays[:, :3]), _cols(rays[:, 3:])
    sun = tuple(np.full(n, F(v), dtype=F) for v in sun_dir)
    with np.errstate(all="ignore"):
        hit, t1, _ = isect_atmosphere(ro, rd)
        march_step = t1 / F(16)
        mu = dot(rd, sun)
        phase_r = F(3) * (ONE + mu * mu) / (F(16) * PI)                         # oracle/ref_lib.h:259
        base = ONE + HG_G * HG_G - F(2) * HG_G * mu                             # :261-263
        phase_m = (ONE - HG_G * HG_G) / ((F(4) + PI) * oracle().math("pow", base, F(1.5)))
        odr = np.zeros(n, dtype=F)
        odm = np.zeros(n, dtype=F)
        sum_r = [np.zeros(n, dtype=F) for _ in range(3)]
        sum_m = [np.zeros(n, dtype=F) for _ in range(3)]
        march_pos = np.zeros(n, dtype=F)
        for _ in range(16):
            s = _sample(ro, rd, march_pos + F(.5) * march_step)
            height = np.sqrt(dot(s, s)) - EARTH_RADIUS
            hr = _exp(-height / HR) * march_step
            hm = _exp(-height / HM) * march_step
            odr = odr + hr
            odm = odm + hm
            over, lr, lm = _sun_light(s, sun)
            for k in range(3):
                tau = BETA_R[k] * (odr + lr) + (BETA_M[k] * F(1.1)) * (odm + lm)
                att = _exp(-tau)
                sum_r[k] = np.where(over, sum_r[k] + hr * att, sum_r[k])
                sum_m[k] = np.where(over, sum_m[k] + hm * att, sum_m[k])
            march_pos = march_pos + march_step
        col = [SUN_POWER * ((sum_r[k] * phase_r) * BETA_R[k] + (sum_m[k] * phase_m) * BETA_M[k]) for k in range(3)]
        return np.stack([np.where(hit, c, ZERO) for c in col], axis=-1).astype(F)


# ---- the ray families (deterministic; directions normalised in float64, then rounded) --------------------------------------------

def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _sphere_dirs(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def family_a(seed=1):
    """40 rays from (0, earth_radius + 1, 0), directions uniform on the sphere (half look down)"""
    rng = np.random.default_rng(seed)
    o = np.tile([0.0, 6360e3 + 1.0, 0.0], (40, 1))
    return np.concatenate([o, _sphere_dirs(rng, 40)], axis=1).astype(F)


def family_b(seed=2):
    """40 rays with origins uniform in the shell earth_radius .. earth_radius + 60 km, any direction"""
    rng = np.random.default_rng(seed)
    r = np.cbrt(rng.uniform(6360e3 ** 3, 6420e3 ** 3, size=(40, 1)))
    return np.concatenate([_sphere_dirs(rng, 40) * r, _sphere_dirs(rng, 40)], axis=1).astype(F)


def family_c(seed=3):
    """20 rays from space (6.5e6 .. 4e7 m from the centre), aimed at and past the planet"""
    rng = np.random.default_rng(seed)
    o = _sphere_dirs(rng, 20) * rng.uniform(6.5e6, 4e7, size=(20, 1))
    target = _sphere_dirs(rng, 20) * rng.uniform(0, 9e6, size=(20, 1))      # inside the planet, in the air, and past the sphere
    return np.concatenate([o, _unit(target - o)], axis=1).astype(F)


def family_d():
    """the awkward ones"""
    re_, ra = 6360e3, 6420e3
    up1 = [0.0, re_ + 1.0, 0.0]
    h = _unit([1.0, 1e-3, .5])
    rows = [
        [0, 0, 0, *_unit([.3, .5, -.2])],                                   # origin at the centre
        [*up1, 0, -1, 0],                                                   # straight down
        [*up1, 0, 1, 0],                                                    # straight up (through the centre line)
        [*up1, 0, 0, 0],                                                    # zero direction
        [*up1, *(2.0 * _unit([.2, .9, .1]))],                               # direction of length 2
        [*up1, *(.5 * _unit([.7, .1, -.4]))],                               # ... and .5
        [*up1, float("nan"), .6, .8],                                       # a NaN direction component
        [float("inf"), re_ + 1.0, 0, 0, .6, .8],                            # an inf origin component
        [*(3e6 * _unit([.1, -.7, .3])), *_unit([.5, .5, .5])],              # origin 3e6 m from the centre
        [*(3e6 * _unit([.1, -.7, .3])), *_unit([.7, .1, -.1])],
        [0, ra, 0, 1, 0, 0],                                                # on the atmosphere sphere, going tangentially
        [0, ra, 0, *_unit([1.0, -1e-3, 0])],                                # ... and dipping in
        [0, re_ - 5e3, 0, *h],                                              # 5 km under the ground, nearly horizontal
        [0, re_ - 5e3, 0, *_unit([1.0, -1e-3, .5])],
    ]
    return np.array(rows, dtype=np.float64).astype(F)


def families():
    """A, B, C, D concatenated -> float32 [n, 6]"""
    return np.concatenate([family_a(), family_b(), family_c(), family_d()], axis=0)


def in_class(rays):
    """the device's qualifying class (csrc/sbx_atmosphere.h atm_eval_class) in the same binary32 operations"""
    rays = _f(rays).reshape(-1, 6)
    ro, rd = _cols(rays[:, :3]), _cols(rays[:, 3:])
    with np.errstate(all="ignore"):
        rc = (ZERO - ro[0], ZERO - ro[1], ZERO - ro[2])
        oo, tca = dot(rc, rc), dot(rc, rd)
        d2 = oo - tca * tca
        return (oo <= ATMOSPHERE_RADIUS * ATMOSPHERE_RADIUS) & (d2 >= F(1e12)) & (np.abs(dot(rd, rd) - ONE) <= F(1e-4))
