"""numpy restatement of SBX_APP_ATMOSPHERE_AIR and sbx_atmosphere_air_eval (include/sbx.h): src/app_atmosphere.h as
shipped with every number it states read from the block sbx_aux_atmosphere_air — the definition of both.  Binary32 step by step on
tests/model_common.py, in the operation order of tests/atmosphere_eval_model.py (whose helpers, ray families and class test it
imports) and tests/atmosphere_ground_model.py (whose plane test it calls with the block's eye and radius); exp, pow, sin, cos, acos
and atan2 are the oracle's.  A block is a dict of the struct's fields; tier_of restates the host's choice of kernel
(csrc/sbx_frames.hip atmosphere_air_tier); _incident_light's optional `witness` says which paths a ray takes through the march and
tile_bodies which body each wave of a run-time launch takes, for the sweep of tests/caller_sweeps.py.  tests/test_atmosphere_air_cpu.py pins the module to the oracle, to the ground model and to
what the reference's own header renders with four blocks written into it (tools/make_golden_atmosphere_airs.py)."""
import os

import numpy as np

from tests import atmosphere_eval_model as E
from tests import atmosphere_ground_model as G
from tests.atmosphere_eval_model import _cols, _exp, _sample
from tests.model_common import F, ONE, ZERO, _f, dot, get_primary_ray, oracle, point_cam, same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIZE, POINTS = (64, 36), 64
INT_FIELDS = ("view", "num_samples", "num_samples_light", "reserved0")
FIELDS = INT_FIELDS + ("eye", "fov", "look_at", "hg_g", "sun_dir", "sun_power", "betaR", "hR", "betaM", "hM", "earth_radius", "atmosphere_radius",
                       "reserved")
SOLVER_FIELDS = ("num_samples", "num_samples_light", "hg_g", "sun_power", "betaR", "hR", "betaM", "hM", "earth_radius", "atmosphere_radius")
LITERAL, RUNTIME, PLAIN = "literal", "run-time", "plain"


def _vec(v):
    return tuple(F(c) for c in v)


def default_air(u_time, view=0):
    """the reference's numbers with the sun setup_scene makes of u_time: sbx_atmosphere_air_default"""
    return dict(view=int(view), num_samples=16, num_samples_light=8, reserved0=0,
                eye=(F(0), E.EARTH_RADIUS + F(1.0), F(0)), fov=F(1.0), look_at=(F(0), E.EARTH_RADIUS + F(1.5), F(-1)), hg_g=E.HG_G,
                sun_dir=_vec(G.sun_dir(u_time)), sun_power=E.SUN_POWER, betaR=E.BETA_R, hR=E.HR, betaM=E.BETA_M, hM=E.HM,
                earth_radius=E.EARTH_RADIUS, atmosphere_radius=E.ATMOSPHERE_RADIUS, reserved=(F(0),) * 6)


def air(u_time=0., view=0, **fields):
    """default_air(u_time, view) with the named fields replaced, each float rounded to binary32 once"""
    A = default_air(u_time, view)
    for k, v in fields.items():
        assert k in FIELDS, k
        A[k] = int(v) if k in INT_FIELDS else _vec(v) if isinstance(A[k], tuple) else F(v)
    return A


def block(A):
    """the 128 bytes of sbx_aux_atmosphere_air as 32 words (uint32)"""
    out = []
    for k in FIELDS:
        if k in INT_FIELDS:
            out.append(np.array([A[k]], dtype=np.int32).view(np.uint32))
        else:
            out.append(np.array(list(A[k]) if isinstance(A[k], tuple) else [A[k]], dtype=F).view(np.uint32))
    out = np.concatenate(out)
    assert out.shape == (32,)
    return out


def of_block(words):
    """block()'s inverse"""
    words = np.asarray(words, dtype=np.uint32)
    A, at = {}, 0
    ref = default_air(0.)
    for k in FIELDS:
        n = len(ref[k]) if isinstance(ref[k], tuple) else 1
        w = words[at:at + n]
        at += n
        A[k] = int(w.view(np.int32)[0]) if k in INT_FIELDS else tuple(w.view(F)) if isinstance(ref[k], tuple) else w.view(F)[0]
    return A


def as_aux(A):
    """the block as the ctypes struct the Python binding takes (shaderbox_amd.AtmosphereAir)"""
    import ctypes

    import shaderbox_amd
    a = shaderbox_amd.AtmosphereAir()
    ctypes.memmove(ctypes.byref(a), block(A).tobytes(), 128)
    return a


def sun(elevation_deg, azimuth_deg):
    """a unit sun `elevation` above the horizon at `azimuth` (from +x towards +z), rounded to binary32"""
    e, a = np.radians(elevation_deg), np.radians(azimuth_deg)
    return _vec((np.cos(e) * np.cos(a), np.sin(e), np.cos(e) * np.sin(a)))


# The fixture blocks (tools/make_golden_atmosphere_airs.py records them, check_conditions says what each must show)
AIRS = {
    "sunset": air(sun_dir=sun(2., 40.)),
    "thin": air(earth_radius=3389.5e3, atmosphere_radius=3389.5e3 + 120e3, hR=11100., hM=3000., betaR=(19.9e-6, 13.6e-6, 5.8e-6),
                betaM=(6e-6, 5e-6, 4e-6), sun_power=9., sun_dir=sun(25., -60.), eye=(0., F(3389.5e3) + F(1.), 0.)),
    "aloft": air(view=1, eye=(0., F(6360e3) + F(20e3), 0.), look_at=(0., F(6360e3) + F(20e3) - F(.15), -1.), fov=1.3, hg_g=.9, sun_power=35.,
                 sun_dir=sun(12., 10.)),
    "coarse": air(num_samples=5, num_samples_light=3, betaM=(30e-6, 21e-6, 12e-6), sun_dir=sun(50., 120.)),
}
POINT_SEEDS = {"sunset": 301, "thin": 302, "aloft": 303, "coarse": 304}


# ---- the host's choice of kernel ----------------------------------------------------------------------------------------------------

def _same(a, b):
    return bool(np.array_equal(np.asarray(a, dtype=F).view(np.uint32), np.asarray(b, dtype=F).view(np.uint32)))


def sun_ok(s):
    with np.errstate(all="ignore"):
        s = _vec(s)
        ss = (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]
        return bool(np.isfinite(np.array(s)).all() and np.abs(ss - ONE) <= F(1e-4))


def default_geometry(A):
    D = default_air(0.)
    return all(_same(A[k], D[k]) for k in ("earth_radius", "atmosphere_radius", "hR", "hM")) and A["num_samples"] == 16 and A["num_samples_light"] == 8


def tame(A):
    """atmosphere_air_tame: the domain of the fast forms (csrc/sbx_atmosphere.h "CALLER'S AIR")"""
    return default_geometry(A) and sun_ok(A["sun_dir"])


def tier_of(A, variant=0, app=True):
    """the tier a launch of the block takes; app=False: sbx_atmosphere_air_eval, which has no literal tier"""
    if variant == 1:
        return PLAIN
    D = default_air(0.)
    solver = default_geometry(A) and all(_same(A[k], D[k]) for k in ("betaR", "betaM", "sun_power", "hg_g"))
    if app and solver and _same(A["eye"], D["eye"]) and (A["view"] == 1 or _same(A["fov"], D["fov"])):
        return LITERAL
    return RUNTIME if tame(A) else PLAIN


def refused(A, app=True):
    """why the entry refuses the block, or None"""
    if app and A["view"] not in (0, 1):
        return "view"
    if not 1 <= A["num_samples"] <= 64:
        return "num_samples"
    if not 1 <= A["num_samples_light"] <= 32:
        return "num_samples_light"
    if A["reserved0"] != 0 or np.asarray(A["reserved"], dtype=F).view(np.uint32).any():
        return "reserved"
    return None


# ---- the solver ---------------------------------------------------------------------------------------------------------------------

def isect_atmosphere(A, ro, rd):                    # isect_sphere :15-26 with sphere (0, atmosphere_radius)
    rc = (ZERO - ro[0], ZERO - ro[1], ZERO - ro[2])
    radius2 = A["atmosphere_radius"] * A["atmosphere_radius"]
    tca = dot(rc, rd)
    d2 = dot(rc, rc) - tca * tca
    thc = np.sqrt(radius2 - d2)
    return d2 < radius2, tca + thc


def _sun_light(A, ro, rd):
    """-> (overground, optical_depthR, optical_depthM), the depths starting at 0 and frozen where the march returned"""
    with np.errstate(all="ignore"):
        _, t1 = isect_atmosphere(A, ro, rd)
        odr = np.zeros(t1.shape, dtype=F)
        odm = np.zeros(t1.shape, dtype=F)
        alive = np.ones(t1.shape, dtype=bool)
        march_pos = np.zeros(t1.shape, dtype=F)
        march_step = t1 / F(A["num_samples_light"])
        for _ in range(A["num_samples_light"]):
            s = _sample(ro, rd, march_pos + F(.5) * march_step)
            height = np.sqrt(dot(s, s)) - A["earth_radius"]
            alive = alive & ~(height < ZERO)
            odr = np.where(alive, odr + _exp(-height / A["hR"]) * march_step, odr)
            odm = np.where(alive, odm + _exp(-height / A["hM"]) * march_step, odm)
            march_pos = march_pos + march_step
        return alive, odr, odm


def get_sun_light(A, rays):
    """rays [n, 6] -> float32 [n, 3] = (overground ? 1 : 0, optical_depthR, optical_depthM)"""
    rays = _f(rays).reshape(-1, 6)
    ok, odr, odm = _sun_light(A, _cols(rays[:, :3]), _cols(rays[:, 3:]))
    return np.stack([np.where(ok, ONE, ZERO), odr, odm], axis=-1).astype(F)


WITNESS = ("tau_in", "tau_out", "od_inf", "under")


def _incident_light(A, ro, rd, witness=None):
    """ro, rd: three float32 arrays [n] each -> float32 [n, 3], the linear RGB of :78-160.  witness: None, or a dict that receives
    one bool [n] per name of WITNESS, the paths the ray takes through the march (all False for a ray that misses the sphere):
      tau_in   a lit sample (its light march did not return) has all three |tau| <= 80: the guard-less exp's side of the fast body's ballot
      tau_out  a lit sample has not (a NaN tau included)
      od_inf   optical_depthR or optical_depthM reaches +inf
      under    a light march returned under the ground
    tau_in, tau_out and under count the samples at which neither optical depth is +inf yet: the ones the fast body's dead-ray exit
    never skips, so that what they say holds of that body whether the exit is on or off."""
    n = len(rd[0])
    ro = tuple(np.broadcast_to(_f(c), (n,)) for c in ro)
    sun_dir = tuple(np.full(n, v, dtype=F) for v in A["sun_dir"])
    g, pi = A["hg_g"], E.PI
    with np.errstate(all="ignore"):
        hit, t1 = isect_atmosphere(A, ro, rd)
        march_step = t1 / F(A["num_samples"])
        mu = dot(rd, sun_dir)
        phase_r = F(3) * (ONE + mu * mu) / (F(16) * pi)
        base = ONE + g * g - F(2) * g * mu
        phase_m = (ONE - g * g) / ((F(4) + pi) * oracle().math("pow", base, F(1.5)))
        odr = np.zeros(n, dtype=F)
        odm = np.zeros(n, dtype=F)
        sum_r = [np.zeros(n, dtype=F) for _ in range(3)]
        sum_m = [np.zeros(n, dtype=F) for _ in range(3)]
        march_pos = np.zeros(n, dtype=F)
        seen = {k: np.zeros(n, dtype=bool) for k in WITNESS}
        for _ in range(A["num_samples"]):
            s = _sample(ro, rd, march_pos + F(.5) * march_step)
            height = np.sqrt(dot(s, s)) - A["earth_radius"]
            hr = _exp(-height / A["hR"]) * march_step
            hm = _exp(-height / A["hM"]) * march_step
            odr = odr + hr
            odm = odm + hm
            over, lr, lm = _sun_light(A, s, sun_dir)
            small = np.ones(n, dtype=bool)
            for k in range(3):
                tau = A["betaR"][k] * (odr + lr) + (A["betaM"][k] * F(1.1)) * (odm + lm)
                small = small & (np.abs(tau) <= F(80))
                att = _exp(-tau)
                sum_r[k] = np.where(over, sum_r[k] + hr * att, sum_r[k])
                sum_m[k] = np.where(over, sum_m[k] + hm * att, sum_m[k])
            seen["od_inf"] |= hit & ((odr == np.inf) | (odm == np.inf))
            live = hit & ~seen["od_inf"]
            seen["tau_in"] |= live & over & small
            seen["tau_out"] |= live & over & ~small
            seen["under"] |= live & ~over
            march_pos = march_pos + march_step
        if witness is not None:
            witness.update(seen)
        col = [A["sun_power"] * ((sum_r[k] * phase_r) * A["betaR"][k] + (sum_m[k] * phase_m) * A["betaM"][k]) for k in range(3)]
        return np.stack([np.where(hit, c, ZERO) for c in col], axis=-1).astype(F)


def get_incident_light(A, rays):
    """rays [n, 6] -> float32 [n, 3] under the block's sun"""
    rays = _f(rays).reshape(-1, 6)
    return _incident_light(A, _cols(rays[:, :3]), _cols(rays[:, 3:]))


# ---- the two builds of render --------------------------------------------------------------------------------------------------------

def dome_dirs(pcx, pcy):                            # :195-202
    m = oracle().math
    with np.errstate(all="ignore"):
        z2 = pcx * pcx + pcy * pcy
        phi = m("atan2", pcy, pcx)
        theta = m("acos", ONE - z2)
        st, ct = m("sin", theta), m("cos", theta)
        return (st * m("cos", phi), ct, st * m("sin", phi))


def parts(A, width, height, fx, fy):
    """linear rgb [n, 3] and the mask of the pixels that are ground (view 1's plane hit) at fragCoords (fx, fy), flat"""
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), A["fov"])
    n = pcx.size
    if A["view"] == 0:
        return _incident_light(A, A["eye"], dome_dirs(pcx, pcy)), np.zeros(n, dtype=bool)
    rd = get_primary_ray(pcx, pcy, A["eye"], A["look_at"])
    sky = G.intersect_plane_t(rd, origin=A["eye"], distance=A["earth_radius"]) > G.MAX_DIST            # :211-220
    col = np.full((n, 3), G.GROUND, dtype=F)                                                          # :223
    if sky.any():
        col[sky] = _incident_light(A, A["eye"], tuple(c[sky] for c in rd))
    return col, ~sky


# ---- which body a wave of the run-time tier takes -------------------------------------------------------------------------------------

SKIPPED, FAST, PLAIN_BODY = 0, 1, 2
CLASS_RAY = (ZERO, E.EARTH_RADIUS + ONE, ZERO, ONE, ZERO, ZERO)      # kern_atmosphere_air.hip air_class_ray


def held_rays(A, width, height):
    """-> (rays float32 [height, width, 6], march bool [height, width]): the ray each pixel's lane holds when its wave votes on the
    class in k_atmosphere_air<VIEW, true> — its own where it marches (view 0: inside the dome's circle, z2 > 2 false; view 1: no plane
    hit), CLASS_RAY where it does not"""
    fx, fy = np.broadcast_arrays(*frame_coords(width, height))
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), A["fov"])
    with np.errstate(all="ignore"):
        if A["view"] == 0:
            march = ~(pcx * pcx + pcy * pcy > F(2))
            rd = dome_dirs(pcx, pcy)
        else:
            rd = get_primary_ray(pcx, pcy, A["eye"], A["look_at"])
            march = G.intersect_plane_t(rd, origin=A["eye"], distance=A["earth_radius"]) > G.MAX_DIST
    rays = np.empty((pcx.size, 6), dtype=F)
    rays[:] = np.array(CLASS_RAY, dtype=F)
    for k in range(3):
        rays[march, k] = F(A["eye"][k])
        rays[march, 3 + k] = rd[k][march]
    return rays.reshape(height, width, 6), march.reshape(height, width)


def tiles_of(a, fill):
    """[height, width, ...] -> [tiles_y, tiles_x, 64, ...]: the 8x8 pixel tiles of pixel_of<8, 1> (csrc/sbx_device.h: lane = 8 * row + column
    within the tile, tile rows from row 0), the lanes past a ragged edge holding `fill`"""
    h, w = a.shape[:2]
    th, tw = (h + 7) // 8, (w + 7) // 8
    full = np.full((th * 8, tw * 8) + a.shape[2:], fill, dtype=a.dtype)
    full[:h, :w] = a
    full = full.reshape((th, 8, tw, 8) + a.shape[2:])
    return np.moveaxis(full, 2, 1).reshape((th, tw, 64) + a.shape[2:])


def tile_bodies(A, width, height):
    """-> int [tiles_y, tiles_x]: what each wave of a tame block's launch does.  A wave is an 8x8 pixel tile; the lanes past a ragged
    edge return before any ballot and have no vote.  SKIPPED: no lane marches (view 0: the whole tile outside the circle; view 1:
    under the horizon) and the wave leaves; FAST: every valid lane's held ray passes E.in_class; PLAIN_BODY otherwise."""
    rays, march = held_rays(A, width, height)
    valid = tiles_of(np.ones((height, width), dtype=bool), False)
    in_class = tiles_of(E.in_class(rays.reshape(-1, 6)).reshape(height, width), False)
    marches = (tiles_of(march, False) & valid).any(axis=-1)
    fast = (in_class | ~valid).all(axis=-1)
    return np.where(~marches, SKIPPED, np.where(fast, FAST, PLAIN_BODY))


def finish(rgb):
    """main.h's linear_to_srgb and alpha 1 -> [n, 4]"""
    out = np.ones((rgb.shape[0], 4), dtype=F)
    with np.errstate(all="ignore"):
        out[:, :3] = oracle().math("pow", np.ascontiguousarray(rgb).ravel(), F(1) / F(2.2)).reshape(rgb.shape)
    return out


def main_image(A, width, height, fx, fy):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    shape = np.broadcast(_f(fx), _f(fy)).shape
    return finish(parts(A, width, height, fx, fy)[0]).reshape(shape + (4,))


def frame_coords(width, height):
    return (np.arange(width, dtype=F) + F(.5))[None, :], (np.arange(height, dtype=F) + F(.5))[:, None]


def frame(A, width, height):
    """float32 [H, W, 4] (row 0 = bottom; fragCoord = pixel centre)"""
    fx, fy = frame_coords(width, height)
    return main_image(A, width, height, fx, fy)


def points(A, width, height, frag):
    frag = np.asarray(frag, dtype=F).reshape(-1, 2)
    return main_image(A, width, height, frag[:, 0], frag[:, 1])


def fixture_points(seed, w, h, n):
    """the n seeded off-centre fragCoords of a fixture"""
    return (np.random.default_rng(seed).uniform(0, 1, size=(n, 2)) * [w, h]).astype(F)


def fixture(name):
    """tests/golden/atmosphere_airs/<name>_WxH.npz: block [32] uint32, frame [h, w, 4], points [n, 2], points_out [n, 4]"""
    return np.load(os.path.join(GOLDEN, "atmosphere_airs", "%s_%dx%d.npz" % (name, SIZE[0], SIZE[1])))


def differing(a, b):
    """the pixels at which two frames differ in a bit"""
    return (~same_bits(a, b)).any(axis=-1)


def ground_mask(A, width, height):
    fx, fy = frame_coords(width, height)
    return parts(A, width, height, fx, fy)[1].reshape(height, width)


def check_conditions(frames, grounds, default_frame):
    """The conditions under which the fixtures say something, over {name: frame}, {name: ground mask} and the default block's frame of
    u_time .37: asserted by the tool that records them, of the reference's own frames, and again of the committed files.  Conditions,
    not measurements."""
    assert set(frames) == set(AIRS) == set(grounds)
    for name, f in frames.items():
        n = f.shape[0] * f.shape[1]
        assert not np.isnan(f).any(), (name, "a NaN pixel")
        lit = (f[..., :3] != 0).any(axis=-1) & ~grounds[name]
        assert lit.sum() >= .40 * n, (name, "lit sky", lit.sum() / n)
        assert differing(f, default_frame).sum() >= .40 * n, (name, "differs from the default block's frame", differing(f, default_frame).sum() / n)
        assert (f[..., 3] == 1).all()
    g = grounds["aloft"].mean()
    assert .3 <= g <= .7, ("aloft: ground share", g)
    assert tame(AIRS["sunset"]) and tier_of(AIRS["sunset"]) == LITERAL


def single_field_airs():
    """{field: (view, block)}: default_air(.37, view) with that field alone changed; look_at in view 1, the rest in view 0"""
    other = dict(num_samples=12, num_samples_light=5, eye=(0., 6365e3, 0.), fov=.8, look_at=(0., F(6360e3) + F(1.9), -1.), hg_g=.6,
                 sun_dir=sun(30., 70.), sun_power=15., betaR=(6e-6, 12e-6, 20e-6), hR=7000., betaM=(18e-6, 21e-6, 25e-6), hM=1500.,
                 earth_radius=6359e3, atmosphere_radius=6430e3)
    assert set(other) == set(FIELDS) - {"view", "reserved0", "reserved"}
    return {k: (1 if k == "look_at" else 0, air(.37, 1 if k == "look_at" else 0, **{k: v})) for k, v in other.items()}
