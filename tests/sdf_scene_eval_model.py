"""sbx_sdf_scene_eval (include/sbx.h): src/app_sdf_ao.h's sdf_normal (:152-163), sdf_ao (:165-181), sdf_shadow (:183-207), illuminate
(:211-243), render_impl (:245-285) and render (:287-311) over elements of the caller's, with sdf(pos) the caller's program, restated in
numpy binary32.  The definition of that entry.

Nothing here is new arithmetic: sdf, sdf_normal, sdf_ao, render_impl and the fog are tests/sdf_scene_model.py's.  What this file adds is
the element form: a direction per ray in sdf_shadow where the app has one sun for all (the loop is restated for direction arrays and
pinned to M.sdf_shadow for a constant one), illuminate on a normal, a material id, an ao and an sh given from outside (the `# illuminate`
block of M.render_impl, lifted out), an origin per ray in render's fog, and the material word of render_impl.  S is the scene dictionary
of tests/sdf_scene_model.py; its eye, look_at and fov are read by primary_rays alone.

THE PORT'S CHOICE: an id outside 0..7 gives the zero colour (the reference's get_material leaves its result unset there).

Pinned from outside (tests/test_sdf_scene_eval_cpu.py): `render` over the primary rays of a fixture scene's frame, followed by the app's
pow(., 1 / 2.2), is the frame the reference's own headers rendered (tests/golden/sdf_scenes/)."""
import numpy as np

from tests import sdf_scene_model as M
from tests.model_common import F, ONE, TWO, ZERO, _f, dot, fmax, fmin, get_primary_ray, oracle, point_cam

WIDTHS = {"sdf": (3, 2), "sdf_normal": (3, 3), "sdf_ao": (6, 1), "sdf_shadow": (6, 1), "illuminate": (9, 3), "render_impl": (6, 5),
          "render": (6, 4)}
FNS = tuple(WIDTHS)


def to_int(x):
    """int() of a material id given as a float: toward zero, saturating at the ends of int, 0 for a NaN (include/sbx.h)"""
    x = _f(x)
    with np.errstate(all="ignore"):
        c = np.clip(np.where(np.isnan(x), ZERO, x).astype(np.float64), -2147483648., 2147483520.)
    return np.trunc(c).astype(np.int64).astype(np.int32)


def cols(x, a, b):
    return tuple(np.ascontiguousarray(x[:, k], dtype=F) for k in range(a, b))


def sdf_shadow(sdf_fn, o, rd, trace=None):
    """sdf_shadow(ray) (:183-207) with a direction per ray: M.sdf_shadow's loop over direction arrays.  trace["exit"]: 0 = the loop ran
    out, 1 = `t > end`, 2 = `d.x < .005`"""
    steps, end, penumbra_factor, darkest = 20, F(20.), F(32.), F(.05)
    o, rd = tuple(_f(c) for c in o), tuple(_f(c) for c in rd)
    n = o[0].size
    t = np.zeros(n, dtype=F)
    umbra = np.ones(n, dtype=F)
    out = np.zeros(n, dtype=F)
    how = np.zeros(n, dtype=np.int8)
    done = np.zeros(n, dtype=bool)
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(steps):
            if act.size == 0:
                break
            ta = t[act]
            d = sdf_fn(o[0][act] + rd[0][act] * ta, o[1][act] + rd[1][act] * ta, o[2][act] + rd[2][act] * ta)[0]
            brk = ta > end
            dark = ~brk & (d < F(.005))
            go = ~brk & ~dark
            out[act[dark]] = darkest
            done[act[dark]] = True
            how[act[dark]] = 2
            how[act[brk]] = 1
            tn = ta[go] + d[go]
            t[act[go]] = tn
            umbra[act[go]] = fmin(umbra[act[go]], penumbra_factor * d[go] / tn)
            act = act[go]
    if trace is not None:
        trace["exit"] = how
    return np.where(done, out, umbra)


def illuminate(S, p, nrm, mat, ao, sh, parts=None):
    """illuminate(eye, hit = (origin p, normal nrm, material mat: int32), ao, sh) (:211-243) -> [n, 3]: the `# illuminate` block of
    M.render_impl.  The reference's eye enters only V (:220), which nothing reads.  parts["parity"]: the checker value of the checker rows"""
    if S["view"]:                                   # :217-219 compiled in
        return np.stack(nrm, axis=1).astype(F)
    sun = tuple(F(x) for x in S["sun_dir"])
    materials = np.asarray(S["materials"], dtype=F)
    with np.errstate(all="ignore"):
        sun_ray = fmax(ZERO, dot(sun, nrm))
        key = sh * sun_ray
        accum = [ZERO + key * c for c in (F(1.2), F(1.3), F(1.))]
        hem = ao * nrm[1]
        accum = [a + hem * c for a, c in zip(accum, (F(.15), F(.15), F(.4)))]
        ind = fmax(ZERO, dot((sun[0] * F(-1), sun[1] * F(0), sun[2] * F(-1)), nrm))
        fill = ao * ind
        accum = [a + fill * c for a, c in zip(accum, (F(.4), F(.28), F(.2)))]
        ok = (mat >= 0) & (mat < len(materials))
        mat_c = np.where(ok[:, None], materials[np.clip(mat, 0, len(materials) - 1)], ZERO).astype(F)
        ground = mat == int(S["checker_material"])
        pat = np.floor(p[0] * F(.5)) + np.floor(p[2] * F(.5))   # checkboard_pattern util.h:95-101
        cb = pat - TWO * np.floor(pat / TWO)
        if parts is not None:
            parts["parity"] = cb[ground]
        lo, hi = mat_c - F(.15) * mat_c, mat_c + F(.15) * mat_c
        mixed = lo * (ONE - cb)[:, None] + hi * cb[:, None]
        mat_c = np.where(ground[:, None], mixed, mat_c)
        return (np.stack(accum, axis=1) * mat_c).astype(F)


def render_impl(S, ro, rd, parts=None):
    """render_impl over rays with an origin each -> (rgb[n, 3], t[n], material id or -1 [n]).  M.render_impl takes one origin for all
    its rays: it runs once per distinct origin (by bits), which is once for a frame's rays.  parts receives M.render_impl's masks at
    full length: hit, left, ran_out, p, mat, and normal (NaN), shadow_exit (-1), parity (-1) where a ray has none"""
    n = rd[0].size
    rgb, t, mat = np.zeros((n, 3), dtype=F), np.zeros(n, dtype=F), np.full(n, -1, dtype=F)
    full = dict(hit=np.zeros(n, dtype=bool), left=np.zeros(n, dtype=bool), ran_out=np.zeros(n, dtype=bool), p=np.zeros((n, 3), dtype=F),
                mat=np.zeros(n, dtype=np.int32), normal=np.full((n, 3), np.nan, dtype=F), shadow_exit=np.full(n, -1, dtype=np.int32),
                parity=np.full(n, -1, dtype=F))
    origins = np.stack(ro, axis=1).astype(F)
    _, first, group = np.unique(origins.view(np.uint32), axis=0, return_index=True, return_inverse=True)
    group = np.asarray(group).reshape(-1)
    for g, k in enumerate(first):
        idx = np.flatnonzero(group == g)
        part = {}
        c, tt = M.render_impl(M.scene_sdf(S), M.renderer_of(S), tuple(origins[k]), tuple(np.ascontiguousarray(d[idx]) for d in rd), part)
        rgb[idx], t[idx] = c, tt
        mat[idx] = np.where(part["hit"], part["mat"], -1)
        for key in ("hit", "left", "ran_out", "p", "mat"):
            full[key][idx] = part[key]
        ih = idx[part["hit"]]
        if "normal" in part:
            full["normal"][ih] = part["normal"]
        if "shadow_exit" in part:
            full["shadow_exit"][ih] = part["shadow_exit"]
        if "parity" in part:
            full["parity"][ih[part["mat"][part["hit"]] == int(S["checker_material"])]] = part["parity"]
    if parts is not None:
        parts.update(full)
    return rgb, t, mat


def fog(S, ro_y, rd_y, rgb, t):
    """render's height fog (:287-311) and the `abs`: M.main_image's arithmetic with the ray's own origin"""
    density, falloff = F(S["fog_density"]), F(S["fog_falloff"])
    o = oracle()
    with np.errstate(all="ignore"):
        e0 = o.math("exp", np.ascontiguousarray(_f(-ro_y * falloff)))
        e1 = o.math("exp", np.ascontiguousarray((-t) * rd_y * falloff))
        f = density * e0 * (ONE - e1) / (rd_y * falloff)
        return np.abs(rgb * (ONE - f)[:, None] + ONE * f[:, None]).astype(F)


def evaluate(fn, S, x, parts=None):
    """the entry: fn over elements x[n, floats in] -> float32 [n, floats out].  parts: a dict for the masks of the function's loop"""
    x = np.ascontiguousarray(x, dtype=F)
    assert x.ndim == 2 and x.shape[1] == WIDTHS[fn][0], (fn, x.shape)
    n = len(x)
    sdf_fn = M.scene_sdf(S)
    with np.errstate(all="ignore"):
        if n == 0:
            return np.zeros((0, WIDTHS[fn][1]), dtype=F)
        if fn == "sdf":
            out = M.sdf(S, *cols(x, 0, 3))
        elif fn == "sdf_normal":
            out = M.sdf_normal(sdf_fn, cols(x, 0, 3))
        elif fn == "sdf_ao":
            out = [M.sdf_ao(sdf_fn, cols(x, 0, 3), cols(x, 3, 6))]
        elif fn == "sdf_shadow":
            out = [sdf_shadow(sdf_fn, cols(x, 0, 3), cols(x, 3, 6), parts)]
        elif fn == "illuminate":
            return illuminate(S, cols(x, 0, 3), cols(x, 3, 6), to_int(x[:, 6]), _f(x[:, 7]), _f(x[:, 8]), parts)
        else:
            rgb, t, mat = render_impl(S, cols(x, 0, 3), cols(x, 3, 6), parts)
            if fn == "render_impl":
                return np.concatenate([rgb, t[:, None], mat[:, None]], axis=1).astype(F)
            return np.concatenate([fog(S, x[:, 1], x[:, 4], rgb, t), t[:, None]], axis=1).astype(F)
        return np.stack([np.broadcast_to(np.asarray(c, dtype=F), (n,)) for c in out], axis=1).astype(F)


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
        out[:, :3] = oracle().math("pow", np.ascontiguousarray(rgb[:, :3], dtype=F).ravel(), F(1) / F(2.2)).reshape(len(rgb), 3)
    return out
