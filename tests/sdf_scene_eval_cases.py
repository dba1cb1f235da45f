"""The element families of sbx_sdf_scene_eval's tests: what tests/test_gpu_sdf_scene_eval.py runs on the device and what
tests/test_sdf_scene_eval_cpu.py holds the conditions of.  A plain module (pytest does not collect it).

    "frame_shadow" ... "frame_short", "frame_ramp"
                    the 2304 primary rays of a 64 x 36 frame of a fixture scene / of the ramp block (u_time .37).  Points, normals, ids, ao
                    and sh are what render_impl has at each hit pixel (ao = sdf_ao there, sh = sdf_shadow(p + sun * .05, sun) under the
                    block's switch, else 1); a miss pixel takes a seeded point near the scene, a seeded unit normal, id, ao and sh.
                    "sdf_shadow" runs the hit pixels' shadow rays and, at the misses, the primary rays themselves
    "seeded"        tame_scene(SEED, 32): 1024 rays from 8 seeded origins (the model's render_impl runs once per origin), points within
                    +-3 of the origin, unit and non-unit directions and normals, ids over -2..9 with fractions, ao and sh in 0..1
    "centres"       CENTRES below: a sphere's centre and points on a cylinder's and a torus's axis, where a root of 0 records; per
                    function the rows that record without a NaN result (the normal AT a sphere's centre is 0 / 0)
    "specials"      a sane row of "frame_shadow"'s scene with NaN, +-inf, 3e38, 1e-40 and -0 in every slot, one slot at a time

family(name, fn) -> inputs [n, floats in of fn]; scene_of(name) -> the scene they are meant for."""
import functools

import numpy as np

from tests import sdf_scene_eval_model as E
from tests import sdf_scene_model as M
from tests.model_common import F

SIZE = (64, 36)
SEED = 3
FRAMES = ("frame_shadow", "frame_plain", "frame_normals", "frame_short", "frame_ramp")
FAMILIES = FRAMES + ("seeded", "centres", "specials")
IDS = (-2, -1, -.5, 0, .9, 1, 2.5, 3, 4, 5, 6, 7, 7.9, 8, 9)

# the ground, a sphere, a y-cylinder (axis y), a torus (axis z) and a box behind the torus's hole; soft shadows on
_mats = np.array([[1, 1, 1], [.2, .6, .2], [.8, .3, .2], [.2, .3, .8], [.7, .7, .2], [.4, .4, .4], [0, 0, 0], [0, 0, 0]], dtype=F)
CENTRES = dict(eye=(F(0), F(3), F(6)), look_at=(F(0), F(1), F(0)), fov=F(.6), march_steps=70, march_end=F(20.), sun_dir=(F(.4), F(.8), F(.4)),
               background=(F(.1), F(.1), F(.7)), shadow=1, view=0, checker_material=1, fog_density=F(.1), fog_falloff=F(.5), materials=_mats,
               program=[M.instr(M.PLANE, (0, 0, 0), (0, 1, 0, 0)), M.obj(1),
                        M.instr(M.SPHERE, (0, 1, 0), (.5,)), M.obj(2),
                        M.instr(M.Y_CYLINDER, (2, 1, 0), (.3, .5)), M.obj(3),
                        M.instr(M.TORUS, (-2, 1, 0), (.6, .2)), M.obj(4),
                        M.instr(M.BOX, (-2, 1, -2), (.4, .4, .25)), M.obj(5)])
assert M.check(CENTRES) is None
# per function, rows that put a field sample exactly on an axis or a centre
_ON = [[0, 1, 0], [2, 1.2, 0], [2, 2.5, 0], [-2, 1, 0], [-2, 1, .75]]          # sphere centre; cylinder axis inside, above; torus axis
CENTRES_ROWS = {
    "sdf": _ON,
    "sdf_normal": _ON[1:],                                                     # (the axes: the taps along the axis stay on it)
    "sdf_ao": [p + n for p in _ON for n in ([0, 0, 0], [0, 1, 0], [0, 0, 1])],
    "sdf_shadow": [p + d for p in _ON for d in ([0, 1, 0], [0, 0, -1], [.4, .8, .4])],
    "illuminate": [p + [0, 1, 0, m, .5, .75] for p in _ON for m in (1, 2, 9)],
    # down the cylinder's axis onto its cap; along the torus's axis through the hole onto the box; the same in steps of 2.5 d; two plain rays
    "render_impl": [[2, 3, 0, 0, -1, 0], [-2, 1, 3, 0, 0, -1], [-2, 1, 3, 0, 0, -2.5], [2, 3.5, 0, 0, -.5, 0], [0, 3, 6, 0, -.3, -1], [1, 2, 4, .1, -.2, -1]],
}
# (a ray along the torus's axis is horizontal, and render's fog of a horizontal ray is 0 / 0: "render" keeps the other four)
CENTRES_ROWS["render"] = [r for r in CENTRES_ROWS["render_impl"] if r[4] != 0]


def scene_of(name):
    if name == "frame_ramp":
        return M.ramp_scene(0.37)
    if name.startswith("frame_"):
        return M.scenes()[name[len("frame_"):]]
    if name == "seeded":
        return M.tame_scene(SEED, 32)
    return CENTRES if name == "centres" else M.scenes()["shadow"]


def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def hit_inputs(S, rays):
    """render_impl's own intermediate values at the hits of rays[n, 6] -> (hit mask, p, normal, id, ao, sh), the last five [n, .] with
    zeros at the misses: what "render_impl" equals the chain of at its own hit points"""
    n = len(rays)
    parts = {}
    E.evaluate("render_impl", S, rays, parts)
    hit = parts["hit"]
    p, nrm, ids = parts["p"].astype(F), np.where(hit[:, None], parts["normal"], 0).astype(F), np.where(hit, parts["mat"], 0).astype(F)
    ao, sh = np.zeros(n, dtype=F), np.ones(n, dtype=F)
    ih = np.flatnonzero(hit)
    if ih.size:
        ao[ih] = E.evaluate("sdf_ao", S, np.concatenate([p[ih], nrm[ih]], axis=1))[:, 0]
        if S["shadow"]:
            sh[ih] = E.evaluate("sdf_shadow", S, shadow_rays(S, p[ih]))[:, 0]
    return hit, p, nrm, ids, ao, sh


def shadow_rays(S, p):
    """the rays render_impl hands sdf_shadow at hit points p[n, 3]: (p + sun * .05, sun) (:271-273)"""
    sun = np.asarray(S["sun_dir"], dtype=F)
    return np.concatenate([p + sun * F(0.05), np.broadcast_to(sun, p.shape)], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def _frame(name):
    S = scene_of(name)
    rays = E.primary_rays(S, *SIZE)
    n = len(rays)
    hit, p, nrm, ids, ao, sh = hit_inputs(S, rays)
    rng = np.random.default_rng(len(name) + n)
    miss = ~hit
    p[miss] = (rng.uniform(-1, 1, size=(n, 3)) * [3, 1.5, 3] + [0, 1.5, 0]).astype(F)[miss]
    nrm[miss] = _unit(rng, n).astype(F)[miss]
    ids[miss] = rng.integers(0, 8, size=n).astype(F)[miss]
    ao[miss] = rng.uniform(0, 1, size=n).astype(F)[miss]
    sh[miss] = rng.uniform(0, 1, size=n).astype(F)[miss]
    shadow = shadow_rays(S, p)
    shadow[miss] = rays[miss]
    return dict(rays=rays, p=p, ao_in=np.concatenate([p, nrm], axis=1), shadow=shadow,
                shade=np.concatenate([p, nrm, ids[:, None], ao[:, None], sh[:, None]], axis=1).astype(F))


@functools.lru_cache(maxsize=None)
def _seeded():
    rng = np.random.default_rng(SEED)
    n = 1024
    ang = rng.uniform(0, 2 * np.pi, size=8)
    eyes = np.stack([4.5 * np.cos(ang), rng.uniform(1, 3, size=8), 4.5 * np.sin(ang)], axis=1)
    o = np.repeat(eyes, n // 8, axis=0)
    aim = rng.uniform(-1, 1, size=(n, 3)) * [2, .8, 2] + [0, .6, 0] - o                # toward the scene, some past it
    d = aim / np.linalg.norm(aim, axis=1, keepdims=True)
    d[n // 2:] *= rng.uniform(.2, 2.5, size=(n - n // 2, 1))                          # half of them are not unit vectors
    p = rng.uniform(-3, 3, size=(n, 3))
    nrm = _unit(rng, n)
    nrm[n // 2:] *= rng.uniform(.2, 2.5, size=(n - n // 2, 1))
    free = _unit(rng, n) * rng.uniform(.2, 2.5, size=(n, 1))                         # shadow rays from the points, any direction
    ids = rng.choice(np.asarray(IDS, dtype=F), size=(n, 1))
    return dict(rays=np.concatenate([o, d], axis=1).astype(F), p=p.astype(F), ao_in=np.concatenate([p, nrm], axis=1).astype(F),
                shadow=np.concatenate([p, free], axis=1).astype(F),
                shade=np.concatenate([p, nrm, ids, rng.uniform(0, 1, size=(n, 2))], axis=1).astype(F))


_KEY = {"sdf": "p", "sdf_normal": "p", "sdf_ao": "ao_in", "sdf_shadow": "shadow", "illuminate": "shade", "render_impl": "rays", "render": "rays"}
# a sane row per function in "frame_shadow"'s scene: a point above the ground, a ray from its eye's side onto the scene
_BASE = {"sdf": [.25, .5, 1], "sdf_normal": [.25, .5, 1], "sdf_ao": [.25, .5, 1, 0, 1, 0], "sdf_shadow": [.25, .5, 1, .4, .8, .4],
         "illuminate": [.25, .5, 1, 0, 1, 0, 2, .5, .75], "render_impl": [.5, 2.5, 6, -.1, -.35, -1], "render": [.5, 2.5, 6, -.1, -.35, -1]}
SPECIAL_VALUES = (np.nan, np.inf, -np.inf, 3e38, 1e-40, -0.)


def family(name, fn):
    """inputs [n, floats in of fn] of a family; the scene they are meant for is scene_of(name)"""
    if name.startswith("frame_"):
        return _frame(name)[_KEY[fn]]
    if name == "seeded":
        return _seeded()[_KEY[fn]]
    if name == "centres":
        return np.array(CENTRES_ROWS[fn], dtype=F)
    rows = [list(_BASE[fn])]
    for k in range(E.WIDTHS[fn][0]):
        for v in SPECIAL_VALUES:
            rows.append(list(_BASE[fn]))
            rows[-1][k] = v
    return np.array(rows, dtype=F)


def roots(fn):
    """whether fn evaluates the field at all: "illuminate" does not, so no wave of it can record"""
    return fn != "illuminate"


def recording_ray():
    """one "render" row of "centres" that records (down the cylinder's axis) for the test of a known re-run"""
    return np.array(CENTRES_ROWS["render"][0], dtype=F)
