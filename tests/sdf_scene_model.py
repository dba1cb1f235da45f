"""SBX_APP_SDF_SCENE and sbx_sdf_eval (include/sbx.h): src/sdf.h's primitives and operators as a postfix program, sphere-traced by the
renderer of src/app_sdf_ao.h, restated in numpy binary32 in the oracle's operation order.  The definition of that app.

A scene is a dictionary

    S = dict(eye=(x, y, z), look_at=(x, y, z), fov=f, march_steps=1..512, march_end=f, sun_dir=(x, y, z), background=(r, g, b),
             shadow=0 | 1, view=0 | 1, checker_material=-1..7, fog_density=f, fog_falloff=f, materials=float32[8, 3],
             program=[dict(op=.., rot_axis=0..3, rot_deg=f, material=0..7, offset=(x, y, z), a=(4), b=(4), c=(4)), ...])

and the program's semantics are those of include/sbx.h: a primitive pushes the reference function's float at q = pos - offset
(rotated by mul(q, rotate_around_*(rot_deg)) if rot_axis != 0), an operator pops d2 then d1 and pushes the float op, OBJECT pops d and
folds vec2(d, float(material)) into the result with the vec2 op_add — `acc.x < v.x ? acc : v`, the later object wins a tie or a NaN.

The renderer takes `sdf` as a parameter (render_frame): with tests/sdf_ao_builds_model.sdf and the shipped constants it is that
model's frame, which is pinned to the oracle and to the reference's own header (tests/test_sdf_scene_cpu.py).  The primitives come
from the models that already state them (sdf_ao: box, y-cylinder and the rotations; egg: Bezier and op_blend; vinyl: capsule); plane,
sphere, torus, the cylinder with P0 != 0 and rotate_around_z's product are stated here."""
import json
import os
import struct

import numpy as np

from tests.egg_builds_model import add3, length3, neg3, op_blend, sd_bezier_x, sub3
from tests.model_common import F, ONE, RADIANS, TWO, ZERO, _f, cross, dot, fmax, fmin, get_primary_ray, normalize, oracle, point_cam
from tests.sdf_ao_builds_model import _mul_rx, _mul_ry, sd_box, sd_y_cylinder
from tests.vinyl_builds_model import sd_capsule

PLANE, SPHERE, BOX, TORUS, Y_CYLINDER, CYLINDER, CAPSULE, BEZIER = range(1, 9)        # SBX_SDF_*
ADD, SUB, INTERSECT, BLEND = 16, 17, 18, 19
OBJECT = 32
PRIMITIVES = (PLANE, SPHERE, BOX, TORUS, Y_CYLINDER, CYLINDER, CAPSULE, BEZIER)
OPERATORS = (ADD, SUB, INTERSECT, BLEND)
MAX_INSTR, MAX_STACK = 32, 4
BLOCK_BYTES, INSTR_BYTES = 2784, 80


def instr(op, offset=(0, 0, 0), a=(0, 0, 0, 0), b=(0, 0, 0, 0), c=(0, 0, 0, 0), rot_axis=0, rot_deg=0.0, material=0):
    pad = lambda v: tuple(F(x) for x in tuple(v) + (0,) * (4 - len(tuple(v))))
    return dict(op=int(op), rot_axis=int(rot_axis), rot_deg=F(rot_deg), material=int(material), offset=tuple(F(x) for x in offset),
                a=pad(a), b=pad(b), c=pad(c))


def obj(material):
    return instr(OBJECT, material=material)


def check(S, program_only=False):
    """the refusals of include/sbx.h, in the C side's order: None if the scene passes, else what is wrong"""
    P = S["program"]
    if not 1 <= len(P) <= MAX_INSTR:
        return "n_instr"
    if not program_only:
        if not -1 <= S["checker_material"] <= 7:
            return "checker_material"
        if not 1 <= S["march_steps"] <= 512:
            return "march_steps"
        if S["shadow"] not in (0, 1):
            return "shadow"
        if S["view"] not in (0, 1):
            return "view"
    depth = 0
    for I in P:
        op = I["op"]
        if op not in PRIMITIVES + OPERATORS + (OBJECT,):
            return "op"
        if not 0 <= I["rot_axis"] <= 3:
            return "rot_axis"
        if op in PRIMITIVES:
            depth += 1
            if depth > MAX_STACK:
                return "overflow"
        elif op in OPERATORS:
            if depth < 2:
                return "underflow"
            depth -= 1
        else:
            if not 0 <= I["material"] <= 7:
                return "material"
            if depth < 1:
                return "underflow"
            depth -= 1
            if depth != 0:
                return "not empty"
    if P[-1]["op"] != OBJECT:
        return "last"
    return None


# ---- the block: struct sbx_aux_sdf_scene ------------------------------------------------------------------------------------------

def to_block(S):
    """the 2784 bytes of an sbx_aux_sdf_scene; unused program slots are zero"""
    f3 = lambda v: [float(F(x)) for x in v]
    b = struct.pack("<3ff", *f3(S["eye"]), float(F(S["fov"])))
    b += struct.pack("<3fi", *f3(S["look_at"]), int(S["march_steps"]))
    b += struct.pack("<3f", *f3(S["sun_dir"])) + np.asarray([S["march_end"]], dtype="<f4").tobytes()
    b += struct.pack("<3fi", *f3(S["background"]), int(S["shadow"]))
    b += np.asarray([S["fog_density"], S["fog_falloff"]], dtype="<f4").tobytes() + struct.pack("<2i", int(S["view"]), int(S["checker_material"]))
    b += struct.pack("<4i", len(S["program"]), 0, 0, 0)
    m = np.zeros((8, 4), dtype="<f4")
    m[:, :3] = np.asarray(S["materials"], dtype=F)
    b += m.tobytes()
    for I in S["program"]:
        b += struct.pack("<2i", I["op"], I["rot_axis"]) + np.asarray([I["rot_deg"]], dtype="<f4").tobytes() + struct.pack("<i", I["material"])
        b += np.asarray(tuple(I["offset"]) + (0,) + tuple(I["a"]) + tuple(I["b"]) + tuple(I["c"]), dtype="<f4").tobytes()
    b += bytes(INSTR_BYTES * (MAX_INSTR - len(S["program"])))
    assert len(b) == BLOCK_BYTES
    return b


def from_block(b):
    b = bytes(b)
    assert len(b) == BLOCK_BYTES
    f = np.frombuffer(b, dtype="<f4")
    i = np.frombuffer(b, dtype="<i4")
    S = dict(eye=tuple(f[0:3]), fov=f[3], look_at=tuple(f[4:7]), march_steps=int(i[7]), sun_dir=tuple(f[8:11]), march_end=f[11],
             background=tuple(f[12:15]), shadow=int(i[15]), fog_density=f[16], fog_falloff=f[17], view=int(i[18]),
             checker_material=int(i[19]), materials=f[24:56].reshape(8, 4)[:, :3].copy(), program=[])
    for k in range(max(0, min(int(i[20]), MAX_INSTR))):
        o = 56 + 20 * k
        S["program"].append(dict(op=int(i[o]), rot_axis=int(i[o + 1]), rot_deg=f[o + 2], material=int(i[o + 3]), offset=tuple(f[o + 4:o + 7]),
                                 a=tuple(f[o + 8:o + 12]), b=tuple(f[o + 12:o + 16]), c=tuple(f[o + 16:o + 20])))
    return S


def as_aux(S):
    """the scene as a shaderbox_amd.SdfScene (the aux block the package's entry points take)"""
    import shaderbox_amd
    return shaderbox_amd.SdfScene.from_buffer_copy(to_block(S))


# ---- sdf(pos) ---------------------------------------------------------------------------------------------------------------------

_SC = {}


def _sincos(deg):
    """(sin, cos) of radians(deg) by the math spec (the oracle's binary32 sin and cos), per distinct bit pattern"""
    key = int(np.asarray(deg, dtype=F).view(np.uint32))
    if key not in _SC:
        with np.errstate(all="ignore"):
            a = _f(F(deg) * RADIANS).reshape(1)
        o = oracle()
        _SC[key] = (o.math("sin", a)[0], o.math("cos", a)[0])
    return _SC[key]


def _mul_rz(p, s, c):                               # mul(p, rotate_around_z): columns (c,-s,0), (s,c,0), (0,0,1)   util.h:44-51
    return ((p[0] * c + p[1] * (-s)) + p[2] * ZERO, (p[0] * s + p[1] * c) + p[2] * ZERO, (p[0] * ZERO + p[1] * ZERO) + p[2] * ONE)


def sd_plane(p, n, d):                              # sdf.h:49-57
    return dot(n, p) + d


def sd_sphere(p, r):                                # sdf.h:59-65
    return length3(p) - r


def sd_torus(p, R, r):                              # sdf.h:75-83
    k = np.sqrt(p[0] * p[0] + p[1] * p[1]) - R
    return np.sqrt(k * k + p[2] * p[2]) - r


def sd_cylinder(P, P0, P1, R):                      # sdf.h:95-109
    d = normalize(sub3(P1, P0))
    dist = length3(cross(d, sub3(P, P0)))
    plane_1 = dot(d, P) + length3(P1)
    plane_2 = dot(neg3(d), P) + (-length3(P0))
    return fmax(fmax(dist, -plane_1), -plane_2) - R


def primitive(I, pos):
    """the float an instruction's primitive returns at pos (arrays)"""
    q = sub3(pos, I["offset"])
    if I["rot_axis"]:
        s, c = _sincos(I["rot_deg"])
        q = (_mul_rx, _mul_ry, _mul_rz)[I["rot_axis"] - 1](q, s, c)
    a, b, c, op = I["a"], I["b"], I["c"], I["op"]
    if op == PLANE:
        return sd_plane(q, a[:3], a[3])
    if op == SPHERE:
        return sd_sphere(q, a[0])
    if op == BOX:
        return sd_box(q, a[:3])
    if op == TORUS:
        return sd_torus(q, a[0], a[1])
    if op == Y_CYLINDER:
        return sd_y_cylinder(q, a[0], a[1])
    if op == CYLINDER:
        return sd_cylinder(q, a[:3], b[:3], a[3])
    if op == CAPSULE:
        return sd_capsule(q, a[:3], b[:3], a[3])
    assert op == BEZIER
    return sd_bezier_x(a[:3], b[:3], c[:3], q, a[3])


def operator(I, d1, d2):
    op = I["op"]
    if op == ADD:
        return fmin(d1, d2)                         # sdf.h:13-18
    if op == SUB:
        return fmax(d1, -d2)                        # :20-28
    if op == INTERSECT:
        return fmax(d1, d2)                         # :30-36
    assert op == BLEND
    return op_blend(d1, d2, I["a"][0])              # :38-47


def sdf(S, px, py, pz, detail=None):
    """sdf(pos) of the scene's program -> (distance, material id as float), arrays like px.  detail: a dict that receives `object`
    (index of the winning OBJECT among the program's objects), `kind` (the primitive kind of the winning object whose own value is
    nearest to 0 there) and `ops` (per object, the set of operators it holds)."""
    with np.errstate(all="ignore"):
        pos = (_f(px), _f(py), _f(pz))
        shape = pos[0].shape
        stack, acc, first = [], None, True
        members, n_obj = [], 0
        win = np.zeros(shape, dtype=np.int32)
        kind = np.zeros(shape, dtype=np.int32)
        ops = []
        cur_ops = set()
        for I in S["program"]:
            if I["op"] in PRIMITIVES:
                d = np.broadcast_to(_f(primitive(I, pos)), shape)
                stack.append(d)
                members.append((I["op"], d))
            elif I["op"] in OPERATORS:
                d2 = stack.pop()
                d1 = stack.pop()
                stack.append(operator(I, d1, d2))
                cur_ops.add(I["op"])
            else:
                d = stack.pop()
                v = (d, np.full(shape, F(I["material"]), dtype=F))
                if first:
                    acc, took = v, np.ones(shape, dtype=bool)
                else:
                    k = acc[0] < v[0]
                    acc, took = (np.where(k, acc[0], v[0]), np.where(k, acc[1], v[1])), ~k
                first = False
                if detail is not None:
                    near = np.argmin(np.stack([np.where(np.isnan(m), np.inf, np.abs(m)) for _, m in members]), axis=0)
                    kinds = np.array([k_ for k_, _ in members], dtype=np.int32)[near]
                    win = np.where(took, n_obj, win)
                    kind = np.where(took, kinds, kind)
                ops.append(cur_ops)
                members, cur_ops, n_obj = [], set(), n_obj + 1
        if detail is not None:
            detail.update(object=win, kind=kind, ops=ops)
        return acc


# ---- the renderer of app_sdf_ao.h over any sdf ------------------------------------------------------------------------------------

def renderer_of(S):
    """the renderer's settings of a scene, as render_frame takes them"""
    return {k: S[k] for k in ("eye", "look_at", "fov", "march_steps", "march_end", "sun_dir", "background", "shadow", "view",
                              "checker_material", "fog_density", "fog_falloff", "materials")}


def sdf_normal(sdf_fn, p):                          # :152-163
    dt = F(0.001)
    with np.errstate(all="ignore"):
        v = (sdf_fn(p[0] + dt, p[1] + ZERO, p[2] + ZERO)[0] - sdf_fn(p[0] - dt, p[1], p[2])[0],
             sdf_fn(p[0] + ZERO, p[1] + dt, p[2] + ZERO)[0] - sdf_fn(p[0], p[1] - dt, p[2])[0],
             sdf_fn(p[0] + ZERO, p[1] + ZERO, p[2] + dt)[0] - sdf_fn(p[0], p[1], p[2] - dt)[0])
        return normalize(v)


def sdf_ao(sdf_fn, origin, normal):                 # :165-181 -> c
    dt = F(.5)
    occlusion = np.zeros(origin[0].shape, dtype=F)
    with np.errstate(all="ignore"):
        for k in range(1, 6):
            i = F(k)
            s = dt * i
            d = sdf_fn(origin[0] + s * normal[0], origin[1] + s * normal[1], origin[2] + s * normal[2])[0]
            pw = oracle().math("pow", _f([2.0]), i)[0]
            occlusion = occlusion + ONE / pw * (dt * i - d)
        return ONE - fmin(fmax(occlusion, ZERO), ONE)


def sdf_shadow(sdf_fn, sun, ox, oy, oz, trace=None):
    """sdf_shadow({origin, sun}) (:183-207); trace["exit"]: 0 = the loop ran out, 1 = `t > end`, 2 = `d.x < .005`"""
    steps, end, penumbra_factor, darkest = 20, F(20.), F(32.), F(.05)
    o = (_f(ox), _f(oy), _f(oz))
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
            d = sdf_fn(o[0][act] + sun[0] * ta, o[1][act] + sun[1] * ta, o[2][act] + sun[2] * ta)[0]
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


def render_impl(sdf_fn, R, ro, rd, parts=None):
    """render_impl (:245-285) for rays (ro, rd[3][n]) -> (rgb[n, 3], t[n]).  parts: a dict that receives the per-ray masks hit, ran_out
    (the loop ended by its count), left (`t > end`), and for the hit rays p, mat, normal, shadow_exit, parity (checker rays)."""
    n = rd[0].size
    t = np.zeros(n, dtype=F)
    hit = np.zeros(n, dtype=bool)
    left = np.zeros(n, dtype=bool)
    mat = np.zeros(n, dtype=np.int32)
    p = [np.zeros(n, dtype=F) for _ in range(3)]
    act = np.arange(n)
    end = F(R["march_end"])
    sun = tuple(F(x) for x in R["sun_dir"])
    materials = np.asarray(R["materials"], dtype=F)
    with np.errstate(all="ignore"):
        for _ in range(int(R["march_steps"])):
            if act.size == 0:
                break
            ta = t[act]
            pi = tuple(ro[k] + rd[k][act] * ta for k in range(3))
            d, m = sdf_fn(*pi)
            brk = ta > end
            h = ~brk & (d < F(.005))
            go = ~brk & ~h
            ih = act[h]
            hit[ih] = True
            left[act[brk]] = True
            mat[ih] = m[h].astype(np.int32)
            for k in range(3):
                p[k][ih] = pi[k][h]
            t[act[go]] = ta[go] + d[go]
            act = act[go]
        rgb = np.empty((n, 3), dtype=F)
        rgb[:] = tuple(F(x) for x in R["background"])
        ih = np.flatnonzero(hit)
        if parts is not None:
            parts.update(hit=hit, left=left, ran_out=~hit & ~left, p=np.stack(p, axis=1), mat=mat)
        if ih.size:
            ph = tuple(c[ih] for c in p)
            nrm = sdf_normal(sdf_fn, ph)
            if parts is not None:
                parts["normal"] = np.stack(nrm, axis=1)
            if R["view"]:                           # illuminate :217-219 compiled in
                rgb[ih] = np.stack(nrm, axis=1)
                return rgb, t
            ao = sdf_ao(sdf_fn, ph, nrm)
            sh = np.ones(ih.size, dtype=F)
            if R["shadow"]:                         # :269-274 compiled in
                tr = {}
                sh = sdf_shadow(sdf_fn, sun, ph[0] + sun[0] * F(0.05), ph[1] + sun[1] * F(0.05), ph[2] + sun[2] * F(0.05), tr)
                if parts is not None:
                    parts["shadow_exit"] = tr["exit"]
            # illuminate :220-242
            sun_ray = fmax(ZERO, dot(sun, nrm))
            key = sh * sun_ray
            accum = [ZERO + key * c for c in (F(1.2), F(1.3), F(1.))]
            hem = ao * nrm[1]
            accum = [a + hem * c for a, c in zip(accum, (F(.15), F(.15), F(.4)))]
            ind = fmax(ZERO, dot((sun[0] * F(-1), sun[1] * F(0), sun[2] * F(-1)), nrm))
            fill = ao * ind
            accum = [a + fill * c for a, c in zip(accum, (F(.4), F(.28), F(.2)))]
            mh = mat[ih]
            ok = (mh >= 0) & (mh < len(materials))
            mat_c = np.where(ok[:, None], materials[np.clip(mh, 0, len(materials) - 1)], ZERO).astype(F)
            ground = mh == int(R["checker_material"])
            pat = np.floor(ph[0] * F(.5)) + np.floor(ph[2] * F(.5))   # checkboard_pattern util.h:95-101
            cb = pat - TWO * np.floor(pat / TWO)
            if parts is not None:
                parts["parity"] = cb[ground]
            lo, hi = mat_c - F(.15) * mat_c, mat_c + F(.15) * mat_c
            mixed = lo * (ONE - cb)[:, None] + hi * cb[:, None]
            mat_c = np.where(ground[:, None], mixed, mat_c)
            rgb[ih] = np.stack(accum, axis=1) * mat_c
    return rgb, t


def main_image(sdf_fn, R, width, height, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4] (main.h over render :287-311)"""
    density, falloff = F(R["fog_density"]), F(R["fog_falloff"])
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), F(R["fov"]))
    eye = tuple(F(x) for x in R["eye"])
    rd = get_primary_ray(pcx, pcy, eye, R["look_at"])
    rgb, t = render_impl(sdf_fn, R, eye, rd, parts)
    o = oracle()
    with np.errstate(all="ignore"):
        e0 = o.math("exp", _f(-eye[1] * falloff).reshape(1))[0]
        e1 = o.math("exp", np.ascontiguousarray((-t) * rd[1] * falloff))
        fog = density * e0 * (ONE - e1) / (rd[1] * falloff)
        col = np.abs(rgb * (ONE - fog)[:, None] + ONE * fog[:, None])
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    out[:, :3] = o.math("pow", np.ascontiguousarray(col).ravel(), F(1) / F(2.2)).reshape(col.shape)
    return out.reshape(shape + (4,))


def render_frame(sdf_fn, R, width, height, parts=None):
    """float32 [H, W, 4] (row 0 = bottom; fragCoord = pixel centre)"""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(sdf_fn, R, width, height, fx, fy, parts)


def scene_sdf(S):
    return lambda x, y, z: sdf(S, x, y, z)


def frame(S, width, height, parts=None):
    return render_frame(scene_sdf(S), renderer_of(S), width, height, parts)


def points(S, width, height, frag):
    frag = np.asarray(frag, dtype=F).reshape(-1, 2)
    return main_image(scene_sdf(S), renderer_of(S), width, height, frag[:, 0], frag[:, 1])


def masks(S, width, height):
    """the per-pixel masks of the frame (flat, row 0 first): hit, ran_out, left, object and kind (nearest object / primitive kind at
    the hit, -1 / 0 elsewhere), shadow_exit (-1 where no shadow march ran), parity (-1 where no checker)"""
    parts = {}
    frame(S, width, height, parts)
    n = width * height
    m = dict(hit=parts["hit"], ran_out=parts["ran_out"], left=parts["left"], object=np.full(n, -1, dtype=np.int32),
             kind=np.zeros(n, dtype=np.int32), shadow_exit=np.full(n, -1, dtype=np.int32), parity=np.full(n, -1, dtype=np.int32), ops=[])
    ih = np.flatnonzero(parts["hit"])
    if ih.size:
        det = {}
        ph = parts["p"][ih]
        sdf(S, ph[:, 0], ph[:, 1], ph[:, 2], det)
        m["object"][ih], m["kind"][ih], m["ops"] = det["object"], det["kind"], det["ops"]
        if "shadow_exit" in parts:
            m["shadow_exit"][ih] = parts["shadow_exit"]
        if "parity" in parts:
            m["parity"][ih[parts["mat"][ih] == int(S["checker_material"])]] = parts["parity"].astype(np.int32)
    return m


# ---- the fixture scenes: tests/golden/sdf_scenes.json (settings only) and tests/golden/sdf_scenes/<name>_64x36.npz -----------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OP_NAMES = {PLANE: "PLANE", SPHERE: "SPHERE", BOX: "BOX", TORUS: "TORUS", Y_CYLINDER: "Y_CYLINDER", CYLINDER: "CYLINDER", CAPSULE: "CAPSULE",
            BEZIER: "BEZIER", ADD: "ADD", SUB: "SUB", INTERSECT: "INTERSECT", BLEND: "BLEND", OBJECT: "OBJECT"}
OP_VALUES = {v: k for k, v in OP_NAMES.items()}
_VEC = ("eye", "look_at", "sun_dir", "background")
_FLT = ("fov", "march_end", "fog_density", "fog_falloff")
_INT = ("march_steps", "shadow", "view", "checker_material")


def entry_of(name, points_seed, S):
    """S -> one entry of the table: every float a hex-float string"""
    hx = lambda v: float(F(v)).hex()  # noqa: E731
    e = dict(name=name, points_seed=int(points_seed))
    e.update({k: [hx(c) for c in S[k]] for k in _VEC})
    e.update({k: hx(S[k]) for k in _FLT})
    e.update({k: int(S[k]) for k in _INT})
    e["materials"] = [[hx(c) for c in m] for m in np.asarray(S["materials"], dtype=F)]
    e["program"] = [dict(op=OP_NAMES[I["op"]], rot_axis=I["rot_axis"], rot_deg=hx(I["rot_deg"]), material=I["material"],
                         offset=[hx(c) for c in I["offset"]], a=[hx(c) for c in I["a"]], b=[hx(c) for c in I["b"]], c=[hx(c) for c in I["c"]])
                    for I in S["program"]]
    return e


def scene_table():
    """the JSON as it is: {"size": [w, h], "points": n, "scenes": [...]}"""
    with open(os.path.join(GOLDEN, "sdf_scenes.json")) as f:
        return json.load(f)


def scene_of(entry):
    x = lambda s: F(float.fromhex(s))  # noqa: E731
    v = lambda p: tuple(x(c) for c in p)  # noqa: E731
    S = {k: v(entry[k]) for k in _VEC}
    S.update({k: x(entry[k]) for k in _FLT})
    S.update({k: int(entry[k]) for k in _INT})
    S["materials"] = np.array([v(m) for m in entry["materials"]], dtype=F)
    S["program"] = [dict(op=OP_VALUES[I["op"]], rot_axis=int(I["rot_axis"]), rot_deg=x(I["rot_deg"]), material=int(I["material"]),
                         offset=v(I["offset"]), a=v(I["a"]), b=v(I["b"]), c=v(I["c"])) for I in entry["program"]]
    assert check(S) is None, entry["name"]
    return S


def scenes():
    """{name: S} of the fixture scenes, in the table's order"""
    return {e["name"]: scene_of(e) for e in scene_table()["scenes"]}


def fixture_points(seed, w, h, n):
    """the n seeded off-centre fragCoords of a fixture"""
    return (np.random.default_rng(seed).uniform(0, 1, size=(n, 2)) * [w, h]).astype(F)


def fixture(name):
    """tests/golden/sdf_scenes/<name>_WxH.npz: frame [h, w, 4], points [n, 2], points_out [n, 4]"""
    w, h = scene_table()["size"]
    return np.load(os.path.join(GOLDEN, "sdf_scenes", "%s_%dx%d.npz" % (name, w, h)))


def check_conditions(table, frames, all_masks):
    """The conditions under which the fixtures say something, over {name: frame} and {name: masks(S, w, h)}, the scenes together:
    asserted by the tool that records them and again of the committed files.  Conditions, not measurements."""
    E = {e["name"]: e for e in table["scenes"]}
    assert len(E) >= 4
    count = lambda f: sum(int(f(m)) for m in all_masks.values())  # noqa: E731
    for kind in PRIMITIVES:
        assert count(lambda m: (m["hit"] & (m["kind"] == kind)).sum()) >= 8, ("primitive kind nearest at fewer than 8 hit pixels", OP_NAMES[kind])
    for op in OPERATORS:
        n = count(lambda m: sum(int((m["hit"] & (m["object"] == j)).sum()) for j, ops in enumerate(m["ops"]) if op in ops))
        assert n >= 8, ("operator in no object that is nearest at 8 hit pixels", OP_NAMES[op])
    assert count(lambda m: (~m["hit"]).sum()) >= 8 and count(lambda m: m["ran_out"].sum()) >= 8 and count(lambda m: m["left"].sum()) >= 8
    for ex in (0, 1, 2):
        assert count(lambda m: (m["shadow_exit"] == ex).sum()) >= 8, ("shadow exit", ex)
    assert count(lambda m: (m["parity"] == 0).sum()) >= 1 and count(lambda m: (m["parity"] == 1).sum()) >= 1
    assert all(not np.isnan(f).any() for f in frames.values()), "a NaN pixel"
    progs = [I for e in E.values() for I in e["program"]]
    assert {I["rot_axis"] for I in progs if OP_VALUES[I["op"]] in PRIMITIVES} >= {1, 2, 3}
    assert {e["shadow"] for e in E.values()} == {0, 1} and any(e["view"] == 1 for e in E.values())
    assert any(e["fov"] != float(1).hex() for e in E.values()) and any(e["march_end"] != float(20).hex() for e in E.values())
    assert any((e["fog_density"], e["fog_falloff"]) != (float(F(.1)).hex(), float(.5).hex()) for e in E.values())
    assert min(e["march_steps"] for e in E.values()) < 70


# ---- the default block (include/sbx.h sbx_sdf_scene_ramp) -------------------------------------------------------------------------

SHIPPED_MATERIALS = np.array([[1, 1, 1], [0, .2, 0], [.1, .1, .1], [.1, .1, .1], [.1, .1, .1], [.4, .4, .4], [0, 0, 0], [0, 0, 0]], dtype=F)


def ramp_scene(u_time):
    """one ramp of sdf_pipe (app_sdf_ao.h:54-113) in sdf_pipe's coordinates and the ground, under the shipped camera for u_time"""
    from tests.sdf_ao_builds_model import camera, sun_dir
    eye, look_at = camera(u_time)
    sx, sy, sz = F(1.3), F(1.), F(1.25)
    o1 = (ZERO, sy, ZERO)
    o2 = (ZERO, sy * TWO, ZERO)
    H = F(-.125)
    P = [instr(BOX, o1, (sx, sy, sz)),
         instr(Y_CYLINDER, add3(o1, (F(.7), F(.5), ZERO)), (sy + F(.55), TWO * sz + F(.1)), rot_axis=1, rot_deg=-90.0),
         instr(SUB), obj(2),
         instr(Y_CYLINDER, add3(o1, (-sx + F(.525), sy, ZERO)), (F(.025), TWO * sz), rot_axis=1, rot_deg=-90.0), obj(5),
         instr(BOX, sub3(o2, (sx, F(-.25), ZERO)), (F(.025), F(.05), sz))]
    bar = lambda z: instr(BOX, sub3(o2, (sx, H, z)), (F(.025), F(.125), F(.025)))
    P += [bar(ZERO), bar(sz / TWO), instr(ADD), bar(sz), instr(ADD), bar(-sz / TWO), bar(-sz), instr(ADD), instr(ADD), instr(ADD), obj(4),
          instr(PLANE, (0, 0, 0), (0, 1, 0, 0)), obj(1)]
    return dict(eye=eye, look_at=look_at, fov=F(1.), march_steps=70, march_end=F(20.), sun_dir=sun_dir(), background=(F(.1), F(.1), F(.7)),
                shadow=0, view=0, checker_material=1, fog_density=F(.1), fog_falloff=F(.5), materials=SHIPPED_MATERIALS.copy(), program=P)


# ---- seeded tame scenes (tests/test_gpu_sdf_scene.py, tools/time_sdf_scene.py) ----------------------------------------------------

def random_primitive(rng, kind, spread=1.6):
    u = lambda lo, hi, n=None: rng.uniform(lo, hi, n).astype(F) if n else F(rng.uniform(lo, hi))
    off = (u(-spread, spread), u(.3, 1.4), u(-spread, spread))
    rot = dict(rot_axis=int(rng.integers(0, 4)), rot_deg=u(-180, 180))
    if kind == PLANE:
        return instr(PLANE, (0, 0, 0), (0, 1, 0, u(-.1, .1)))
    if kind == SPHERE:
        return instr(SPHERE, off, (u(.3, .8),), **rot)
    if kind == BOX:
        return instr(BOX, off, tuple(u(.25, .7, 3)), **rot)
    if kind == TORUS:
        return instr(TORUS, off, (u(.4, .8), u(.1, .25)), **rot)
    if kind == Y_CYLINDER:
        return instr(Y_CYLINDER, off, (u(.2, .6), u(.5, 1.5)), **rot)
    if kind == CYLINDER:
        return instr(CYLINDER, off, tuple(u(-.3, .1, 3)) + (u(.1, .3),), tuple(u(.3, 1, 3)), **rot)
    if kind == CAPSULE:
        return instr(CAPSULE, off, tuple(u(-.6, 0, 3)) + (u(.1, .3),), tuple(u(.1, .8, 3)), **rot)
    return instr(BEZIER, off, tuple(u(-.9, -.3, 3)) + (u(.08, .2),), (u(-.2, .2), u(.4, .9), u(-.2, .2)), tuple(u(.2, .7, 3)), **rot)


def tame_scene(seed, n_instr=None, march_steps=70):
    """a seeded scene of finite, moderate numbers.  n_instr is even (an object of k primitives takes 2k instructions: k primitives,
    k - 1 operators, its OBJECT), 2..32; every fourth primitive group is bushy, so that the stack reaches 4."""
    rng = np.random.default_rng(seed)
    if n_instr is None:
        n_instr = 2 * int(rng.integers(2, 17))
    assert n_instr % 2 == 0 and 2 <= n_instr <= MAX_INSTR
    P = [instr(PLANE, (0, 0, 0), (0, 1, 0, 0)), obj(1)]
    left = n_instr // 2 - 1
    j = 0
    while left > 0:
        k = int(min(left, rng.integers(1, 5)))
        prims = [random_primitive(rng, int(rng.choice(PRIMITIVES[1:]))) for _ in range(k)]
        anchor = prims[0]["offset"]                 # the members of an object stay near each other, so that the operators matter
        for q in prims[1:]:
            q["offset"] = tuple(F(a + F(rng.uniform(-.35, .35))) for a in anchor)
        mk = lambda: instr(int(rng.choice(OPERATORS)), a=(F(rng.uniform(.05, .4)),))
        if k == 4 and j % 2 == 0:                   # bushy: depth 4
            P += prims + [mk(), mk(), mk()]
        else:
            P += [prims[0]]
            for q in prims[1:]:
                P += [q, mk()]
        P.append(obj(int(rng.integers(0, 8))))
        left -= k
        j += 1
    ang = rng.uniform(0, 2 * np.pi)
    mats = rng.uniform(.05, 1, (8, 3)).astype(F)
    S = dict(eye=(F(4.5 * np.cos(ang)), F(rng.uniform(1.5, 3)), F(4.5 * np.sin(ang))), look_at=(F(0), F(rng.uniform(.3, 1)), F(0)),
             fov=F(rng.uniform(.35, .6)), march_steps=int(march_steps), march_end=F(rng.uniform(12, 25)),
             sun_dir=tuple(rng.uniform(.2, 1, 3).astype(F)), background=tuple(rng.uniform(0, 1, 3).astype(F)),
             shadow=int(rng.integers(0, 2)), view=0, checker_material=int(rng.integers(-1, 8)), fog_density=F(rng.uniform(0, .2)),
             fog_falloff=F(rng.uniform(.2, .8)), materials=mats, program=P)
    assert check(S) is None and len(P) == n_instr
    return S


def depth_of(S):
    d = m = 0
    for I in S["program"]:
        d += 1 if I["op"] in PRIMITIVES else -1
        m = max(m, d)
    return m
