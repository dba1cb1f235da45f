"""sbx_raytracer_eval (include/sbx.h): src/app_raytracer.h's raytrace_iteration (:70-86), illuminate (:46-68), the shadow test
(:109-116) and render (:88-136) over elements of the caller's, restated in numpy binary32.  The definition of that entry.

Nothing here is new arithmetic: trace, material, fresnel_factor, the two lighting models and normalize are
tests/raytracer_builds_model.py's, illuminate is tests/raytracer_scene_model.py's; what this file adds is the element form — an origin
per ray where the scene app has one eye, a mat_to_ignore per ray, a hit given from outside — and the depth count.  S is the scene
dictionary of tests/raytracer_scene_model.py; its eye, look_at and fov are not read.

Pinned from outside (tests/test_raytracer_eval_cpu.py): `render` over the primary rays of a fixture scene's frame, followed by the
app's pow(., 1 / 2.2), is the frame that the reference's own headers rendered (tests/golden/raytracer_scenes/)."""
import numpy as np

from tests.model_common import F, ONE, TWO, ZERO, _f, dot, get_primary_ray, point_cam  # noqa: F401
from tests.raytracer_builds_model import BIAS, MAX_DIST, _math, fresnel_factor, material, normalize, trace
from tests.raytracer_scene_model import illuminate

WIDTHS = {"raytrace_iteration": (7, 8), "illuminate": (10, 3), "shadow": (3, 2), "render": (6, 4)}
FNS = tuple(WIDTHS)


def to_int(x):
    """int() of a material id given as a float: toward zero, saturating at the ends of int, 0 for a NaN (include/sbx.h)"""
    x = _f(x)
    with np.errstate(all="ignore"):
        c = np.clip(np.where(np.isnan(x), ZERO, x).astype(np.float64), -2147483648., 2147483520.)
    return np.trunc(c).astype(np.int64).astype(np.int32)


def cols(x, a, b):
    return [np.ascontiguousarray(x[:, k], dtype=F) for k in range(a, b)]


def raytrace_iteration(S, ro, rd, ignore):
    """trace with a mat_to_ignore per ray (int32 array) -> t, material id, normal, origin.  trace takes one id for all rays: it runs
    once per id that some sphere carries and some ray names, and once with an id that no sphere carries for the rest."""
    ignore = np.asarray(ignore, dtype=np.int32)
    carried = sorted({int(m) for _, _, m in S["spheres"]})
    none = next(v for v in range(-2, -2 - len(carried) - 2, -1) if v not in carried)
    t, mat, nor, org = trace(S, ro, rd, none)
    for v in carried:
        pick = ignore == v
        if not pick.any():
            continue
        tv, mv, nv, ov = trace(S, ro, rd, v)
        t, mat = np.where(pick, tv, t), np.where(pick, mv, mat)
        nor = [np.where(pick, nv[k], nor[k]) for k in range(3)]
        org = [np.where(pick, ov[k], org[k]) for k in range(3)]
    return t, mat, nor, org


def shadow(S, org):
    """:109-116 at hit.origin = org -> (shadow_hit.t, length(shadow_line)); lights[0].L - hit.origin whatever the light's type"""
    line = [S["light"][k] - org[k] for k in range(3)]
    sdir = normalize(line)
    st = trace(S, [org[k] + sdir[k] * BIAS for k in range(3)], sdir, 0)[0]
    return st, np.sqrt(dot(line, line))


def render(S, ro, rd):
    """:88-136 over the rays (ro, rd), three float32 arrays each -> (linear colour, depth): tests/raytracer_scene_model.py's render with
    the ray's own origin as the primary origin of :105"""
    n = rd[0].shape
    eye = [np.asarray(v, dtype=F) for v in ro]
    ro, rd = list(eye), [np.asarray(v, dtype=F) for v in rd]
    color = [np.zeros(n, dtype=F) for _ in range(3)]
    accum = [np.ones(n, dtype=F) for _ in range(3)]
    active = np.ones(n, dtype=bool)
    depth = np.zeros(n, dtype=np.int32)
    for i in range(int(S["bounces"])):
        t, mat, nor, org = trace(S, ro, rd, -1)
        miss = active & (t >= MAX_DIST)
        live = active & ~miss
        depth = depth + live
        f = fresnel_factor(ONE, ONE, dot(nor, [-rd[k] for k in range(3)]))
        ill, _ = illuminate(S, eye, mat, nor, org)
        for k in range(3):
            color[k] = np.where(miss, color[k] + accum[k] * ZERO, color[k])              # background :13-16
            color[k] = np.where(live, color[k] + ((ONE - f) * accum[k]) * ill[k], color[k])
        if i == 0 and S["shadow"]:
            st, reach = shadow(S, org)
            for k in range(3):
                color[k] = np.where(live & (st < reach), color[k] * F(0.1), color[k])
        refl = live & (material(S, mat)[3] > ZERO)
        s = TWO * dot(rd, nor)                          # reflect(hit.normal, ray.direction): arguments swapped in the reference (:127)
        rdir = normalize([nor[k] - s * rd[k] for k in range(3)])
        for k in range(3):
            accum[k] = np.where(refl, accum[k] * f, accum[k])
            ro[k] = np.where(refl, org[k] + rdir[k] * BIAS, ro[k])
            rd[k] = np.where(refl, rdir[k], rd[k])
        active = refl
    return color, depth


def evaluate(fn, S, x):
    """the entry: fn over elements x[n, floats in] -> float32 [n, floats out]"""
    x = np.ascontiguousarray(x, dtype=F)
    assert x.ndim == 2 and x.shape[1] == WIDTHS[fn][0], (fn, x.shape)
    with np.errstate(all="ignore"):
        if fn == "raytrace_iteration":
            t, mat, nor, org = raytrace_iteration(S, cols(x, 0, 3), cols(x, 3, 6), to_int(x[:, 6]))
            out = [t, mat.astype(F)] + org + nor
        elif fn == "illuminate":
            out = illuminate(S, cols(x, 0, 3), to_int(x[:, 9]), cols(x, 6, 9), cols(x, 3, 6))[0]
        elif fn == "shadow":
            out = shadow(S, cols(x, 0, 3))
        else:
            color, depth = render(S, cols(x, 0, 3), cols(x, 3, 6))
            out = color + [depth.astype(F)]
        return np.stack([np.broadcast_to(np.asarray(c, dtype=F), (len(x),)) for c in out], axis=1).astype(F)


def primary_rays(S, w, h):
    """[w * h, 6]: the primary rays of S's own camera over a w x h frame, row 0 = bottom (the app's rays, origin = S's eye)"""
    fx = np.tile(np.arange(w, dtype=F) + F(.5), h)
    fy = np.repeat(np.arange(h, dtype=F) + F(.5), w)
    pcx, pcy = point_cam(w, h, fx, fy, F(S["fov"]))
    rd = get_primary_ray(pcx, pcy, S["eye"], S["look_at"])
    return np.stack([np.full(w * h, F(S["eye"][k])) for k in range(3)] + [np.asarray(rd[k], dtype=F) for k in range(3)], axis=1).astype(F)


def finish(rgb):
    """the app's last step over linear colours [n, 3] -> [n, 4]: pow(., 1 / 2.2) and alpha 1 (main.h:52)"""
    out = np.ones((len(rgb), 4), dtype=F)
    with np.errstate(all="ignore"):
        for k in range(3):
            out[:, k] = _math("pow", np.ascontiguousarray(rgb[:, k]), F(1) / F(2.2))
    return out
