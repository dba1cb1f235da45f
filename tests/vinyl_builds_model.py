"""numpy restatement of the four builds of src/app_vinyl.h: SBX_APP_VINYL ("default", as shipped), SBX_APP_VINYL_CLOSEUP ("closeup",
the `#if 1` of setup_camera at :60 turned to `#if 0`: eye and look_at of :64-65), SBX_APP_VINYL_RIDGES ("ridges", the `#if 0` of
illuminate at :357 on: the ridge of :358-363 on label and logo hits) and SBX_APP_VINYL_NOSHADOW ("noshadow", the `#if 1` of render
at :445 off: sh stays 1.); include/sbx.h, DESIGN.md §5.15.  All four with the C++ build's 60 march steps (:411-416).

The CPU oracle renders the shipped build only and is not to grow, so the GPU tests of the three other builds compare against this
module.  It is pinned from two sides (tests/test_vinyl_builds_cpu.py): build "default" equals Oracle.render("vinyl") in every bit —
which covers everything the four builds share: camera arithmetic, sdf_logo, platter, tonearm, the unions, the march, sdf_shadow,
sdf_normal, both shading branches, epilogue — and the other three equal frames and points that the reference header itself rendered
with the one line edited (tests/golden/vinyl_builds/, tools/make_golden_builds.py), NaN pixels included.

mainImage -> render -> sdf / sdf_shadow / illuminate, vectorised over pixels, in binary32 step by step in the oracle's operation
order (oracle/ovec.h: dot = (x x + y y) + z z, normalize = three divisions by sqrtf, v * M = the three dots with M's columns,
A * B column by column; oracle/sbx_math_ref.h: min / max as compare-and-select, mix = x (1 - a) + y a), every value an explicit
np.float32.  sin, cos, exp, pow and noise_iq are the oracle's (Oracle.math, Oracle.noise).  What depends on u_time alone (the platter
and wobble rotations) and on nothing (the tonearm's constant frames) is evaluated once (`scene`), in the same operations.  The vector
algebra and the camera are tests/model_common.py's; the primitives sd_cylinder and sd_bezier are tests/egg_builds_model.py's.
"""
import functools

import numpy as np

from tests.egg_builds_model import add3, clamp, length3, mat_vec, sd_bezier_x, sd_cylinder, sub3
from tests.model_common import (F, ONE, RADIANS, TWO, ZERO, _const, _f, builds_fixture, cross, dot, fmax, fmin, get_primary_ray,
                                 normalize, op_add2, oracle, point_cam, same_bits)

BUILDS = ("default", "closeup", "ridges", "noshadow")
APP_OF = {"default": "vinyl", "closeup": "vinyl_closeup", "ridges": "vinyl_ridges", "noshadow": "vinyl_noshadow"}
# setup_camera :56-67: (eye, look_at); the `#else` pair for closeup
CAMERA = {b: ((F(0), F(5.75), F(6.75)), (F(0), F(-2.5), F(0))) for b in BUILDS}
CAMERA["closeup"] = ((F(-2), F(1.5), F(5.5)), (F(-1.5), F(0), F(0)))
FOV = F(1.)                                         # :460
STEPS = 60                                          # :411-416, the __cplusplus value
MAT_GROOVE, MAT_DEAD_WAX, MAT_LABEL, MAT_LOGO, MAT_SHINY = 1, 2, 3, 4, 5      # :20-24
BASE_COLOR = {0: (F(1), F(1), F(1)), MAT_GROOVE: (F(.01), F(.01), F(.01)), MAT_DEAD_WAX: (F(.05), F(.05), F(.05)),
              MAT_LABEL: (F(.5), F(.5), F(.0)), MAT_LOGO: (F(0), F(0), F(.7)), MAT_SHINY: (F(.7), F(.7), F(.7))}   # setup_scene :40-54
PI = F(3.14159265359)                               # def.h:51


def _sincos_rad(a):
    a = _f(a).reshape(1)
    o = oracle()
    return o.math("sin", a)[0], o.math("cos", a)[0]


def rotate_around_x(deg):                           # util.h:62-69; columns
    s, c = _sincos_rad(F(deg) * RADIANS)
    return ((ONE, ZERO, ZERO), (ZERO, c, -s), (ZERO, s, c))


def rotate_around_y(deg):                           # util.h:53-60
    s, c = _sincos_rad(F(deg) * RADIANS)
    return ((c, ZERO, s), (ZERO, ONE, ZERO), (-s, ZERO, c))


def rotate_around_z(deg):                           # util.h:44-51
    s, c = _sincos_rad(F(deg) * RADIANS)
    return ((c, -s, ZERO), (s, c, ZERO), (ZERO, ZERO, ONE))


def vec_mat(v, m):
    """v * M for columns m: (dot(v, c0), dot(v, c1), dot(v, c2)) (oracle/ovec.h:94)"""
    return (dot(v, m[0]), dot(v, m[1]), dot(v, m[2]))


def mat_mat(a, b):
    """A * B: column j is A * (column j of B) (oracle/ovec.h:96-100)"""
    return tuple(mat_vec(a, b[j]) for j in range(3))


def scale3(v, s):
    return (v[0] * s, v[1] * s, v[2] * s)


def length2(x, y):
    return np.sqrt(x * x + y * y)


def sd_box(p, b):                                   # sdf.h:67-73
    return fmax(np.abs(p[0]) - b[0], fmax(np.abs(p[1]) - b[1], np.abs(p[2]) - b[2]))


def sd_y_cylinder(p, r, h):                         # sdf.h:85-93
    return fmax(length2(p[0], p[2]) - r, np.abs(p[1]) - h / TWO)


def sd_capsule(p, a, b, r):                         # sdf.h:162-171
    ab = sub3(b, a)
    t = clamp(dot(sub3(p, a), ab) / dot(ab, ab), ZERO, ONE)
    return length3(sub3(add3(scale3(ab, t), a), p)) - r


def op_sub(d1, d2):                                 # sdf.h:20-28
    return fmax(d1, -d2)


def saw(x):                                         # :274-277
    return x - np.floor(x)


def pulse(x):                                       # :279-282
    return saw(x + F(.5)) - saw(x)


# ---- the scene -----------------------------------------------------------------------------------------------------------

_CONST = {}
_SCENES = {}


def constants():
    """the frames of sdf_logo and sdf_tonearm that depend on nothing (:75-81, :144-238)"""
    if not _CONST:
        with np.errstate(all="ignore"):
            C = _CONST
            C["ry30"], C["rym30"] = rotate_around_y(30.), rotate_around_y(-30.)
            C["sun_dir"] = normalize((F(-1), F(4), F(-3)))                               # :284-285
            H = F(.8)
            C["base_p"] = (F(-7), F(0), F(-5))
            C["a0"] = add3(C["base_p"], (F(-1), H, F(-2)))
            C["a1"], C["a11"], C["a2"] = (F(-6), H, F(-3)), (F(-4.25), H, F(2)), (F(-4.1), H, F(2.45))
            C["a33"], C["a3"] = (F(-3.5), H, F(3)), (F(-2), H, F(4))
            fwd = normalize(sub3(C["a3"], C["a33"]))
            up = (ZERO, ONE, ZERO)
            right = cross(fwd, up)
            C["arm_fwd"], C["arm_up"], C["arm_right"] = fwd, up, right
            C["arm_xform"] = (fwd, up, right)
            C["fl_rot"] = mat_mat(C["arm_xform"], rotate_around_x(45.))
            C["fl_rot2"] = rotate_around_x(-45.)
            C["ctg_rot"] = rotate_around_z(44.)
            C["cut_rx10"], C["cut_rym5"], C["cut2_rz10"] = rotate_around_x(10.), rotate_around_y(-5.), rotate_around_z(10.)
    return _CONST


def scene(u_time):
    """what render and sdf_tonearm compute from u_time alone: platter_rot (:419-428) and the wobble (:141-142)"""
    key = np.asarray(u_time, dtype=F).tobytes()
    if key not in _SCENES:
        with np.errstate(all="ignore"):
            t = F(u_time)
            o = oracle()
            s1 = o.math("sin", _f(t).reshape(1))[0]
            s2 = o.math("sin", _f(t * F(3.6758)).reshape(1))[0]
            S = {"platter_rot": mat_mat(rotate_around_y(t * F(200.)), rotate_around_x(s1 * F(.1))),
                 "wobble": rotate_around_x(s2 * F(.1))}
        if len(_SCENES) > 64:
            _SCENES.clear()
        _SCENES[key] = S
    return _SCENES[key]


def sdf_logo(pos, thick):                           # :71-87
    C = constants()
    b = (F(.25), thick, F(1.2))
    d = (F(.7), ZERO, ZERO)
    v1 = sd_box(sub3(vec_mat(pos, C["ry30"]), d), b)
    v2 = sd_box(add3(vec_mat(pos, C["rym30"]), d), b)
    x = sd_box(pos, (F(1.5), thick, F(1.35)))
    return fmax(fmin(v1, v2), x)                    # op_intersect(op_add(v1, v2), x)


def sdf_platter(p):                                 # :89-125 -> (distance, material)
    thick = F(.1)
    like = p[0]
    lead_in = (sd_y_cylinder(p, F(6.), thick - F(.05)), _const(MAT_DEAD_WAX, like))
    groove = (sd_y_cylinder(p, F(5.9), thick), _const(MAT_GROOVE, like))
    dead_wax = (sd_y_cylinder(p, F(3.), thick), _const(MAT_DEAD_WAX, like))
    label = (sd_y_cylinder(p, F(2.), thick), _const(MAT_LABEL, like))
    logo = (sdf_logo(p, thick - F(.0175)), _const(MAT_LOGO, like))
    spc = sd_y_cylinder(p, F(.10), F(.6))
    sps = length3(sub3(p, (ZERO, F(.3), ZERO))) - F(.10)
    spindle = (fmin(spc, sps), _const(MAT_SHINY, like))
    d0 = op_add2(groove, lead_in)
    d1 = op_add2(d0, dead_wax)
    d2 = op_add2(label, logo)
    d3 = op_add2(d1, d2)
    d4 = op_add2(d3, spindle)
    defect1 = length3(add3(p, (F(6.05), ZERO, ZERO))) - F(.1)
    defect2 = length3(add3(p, (F(-6.05), ZERO, ZERO))) - F(.1)
    defect = fmin(defect1, defect2)
    return op_sub(d4[0], defect), d4[1]


def sdf_tonearm(S, pos):                            # :127-249
    C = constants()
    like = pos[0]
    shiny = _const(MAT_SHINY, like)
    base_p = C["base_p"]
    q = sub3(pos, base_p)
    platter = sd_y_cylinder(pos, F(6.25), F(1.))
    base_0 = sd_y_cylinder(q, F(3.), F(.25))
    base_1 = op_sub(base_0, platter)
    base_2 = sd_y_cylinder(q, F(1.25), F(1.))
    base_12 = fmin(base_1, base_2)
    base = op_add2((base_12, shiny), (sd_y_cylinder(q, F(0.5), F(2.5)), shiny))

    p = vec_mat(pos, S["wobble"])
    R = F(.1)
    arm1 = sd_capsule(p, C["a0"], C["a1"], R)
    arm2 = sd_capsule(p, C["a1"], C["a11"], R)
    arm3 = sd_capsule(p, C["a33"], C["a3"], R)
    armb = sd_bezier_x(C["a11"], C["a2"], C["a33"], p, R)
    arm_link1 = fmin(arm1, arm2)
    arm_link2 = fmin(arm_link1, arm3)
    arm = (fmin(arm_link2, armb), shiny)

    fwd, up, right = C["arm_fwd"], C["arm_up"], C["arm_right"]
    clr_p = sub3(p, C["a3"])
    clr_r = R * F(1.5)
    zero = (ZERO, ZERO, ZERO)
    collar = sd_cylinder(clr_p, add3(zero, scale3(fwd, F(.05))), clr_r)

    fl_w, fl_h = F(.045), F(.020)
    fl_len1 = clr_r * F(1.)
    fl_len2 = fl_len1 * F(1.2)
    fl_p = vec_mat(sub3(sub3(clr_p, scale3(right, clr_r)), scale3(up, clr_r)), C["fl_rot"])
    fl1 = sd_box(fl_p, (fl_w, fl_h, fl_len1))
    fl2 = sd_box(sub3(vec_mat(sub3(fl_p, (ZERO, ZERO, fl_len1)), C["fl_rot2"]), (ZERO, ZERO, fl_len2)), (fl_w, fl_h, fl_len2))
    finger_lift = fmin(fl1, fl2)
    headshell = (fmin(collar, finger_lift), shiny)

    ctg_w, ctg_h, ctg_len1, ctg_len2 = F(.05), F(.05), F(.3), F(.5)
    ctg_p = vec_mat(clr_p, C["arm_xform"])
    ctg1 = sd_box(ctg_p, (ctg_len1, ctg_h, ctg_w))
    ctg2_p = sub3(vec_mat(sub3(ctg_p, (ctg_len1, ZERO, ZERO)), C["ctg_rot"]), (ctg_len2 - F(0.03), F(-.01), ZERO))
    ctg2 = sd_box(ctg2_p, (ctg_len2, ctg_h, ctg_w))
    cut = sd_box(vec_mat(sub3(vec_mat(ctg2_p, C["cut_rx10"]), (ZERO, F(.05), F(.175))), C["cut_rym5"]),
                 (ctg_len2 * F(2.), ctg_h * F(3.), ctg_w * F(3.2)))
    cut2 = sd_box(vec_mat(sub3(ctg2_p, (F(.3), F(.2), ZERO)), C["cut2_rz10"]), (F(.4), F(.2), F(.3)))
    ctg12 = fmin(ctg1, ctg2)
    ctg12c = op_sub(ctg12, cut)
    cartridge = (op_sub(ctg12c, cut2), shiny)

    tone1 = op_add2(base, arm)
    tone2 = op_add2(headshell, cartridge)
    return op_add2(tone1, tone2)


def sdf(build, u_time, px, py, pz):
    """sdf(pos) (:251-259) -> (distance, material id as float), arrays like px.  No build enters: the four builds share the scene."""
    assert build in BUILDS, build
    S = scene(u_time)
    with np.errstate(all="ignore"):
        pos = (_f(px), _f(py), _f(pz))
        plat = sdf_platter(vec_mat(pos, S["platter_rot"]))
        arm = sdf_tonearm(S, pos)
        return op_add2(plat, arm)


def sdf_normal(build, u_time, p):                   # :261-272
    dt = F(0.001)

    def d(k, sign):
        q = [p[0], p[1], p[2]]
        q[k] = q[k] + dt if sign > 0 else q[k] - dt
        return sdf(build, u_time, *q)[0]

    return normalize((d(0, 1) - d(0, -1), d(1, 1) - d(1, -1), d(2, 1) - d(2, -1)))


def sdf_shadow(build, u_time, ox, oy, oz):
    """sdf_shadow({origin, sun_dir}) (:381-405), the statements of :391-401 in their order"""
    o = (_f(ox), _f(oy), _f(oz))
    dr = constants()["sun_dir"]
    n = o[0].size
    t = np.zeros(n, dtype=F)
    umbra = np.ones(n, dtype=F)
    dark = np.zeros(n, dtype=bool)
    act = np.arange(n)
    with np.errstate(all="ignore"):
        for _ in range(20):
            if act.size == 0:
                break
            ta = t[act]
            d = sdf(build, u_time, o[0][act] + dr[0] * ta, o[1][act] + dr[1] * ta, o[2][act] + dr[2] * ta)[0]
            brk = ta > F(5.)
            hit = ~brk & (d < F(.005))
            go = ~brk & ~hit
            dark[act[hit]] = True
            tn = ta[go] + d[go]
            t[act[go]] = tn
            umbra[act[go]] = fmin(umbra[act[go]], F(16.) * d[go] / tn)
            act = act[go]
    return np.where(dark, F(.05), umbra).astype(F)


def illuminate(build, u_time, eye, p, mat):
    """illuminate(eye, hit) (:287-379) for hits p[3][n] of material ids mat[n] -> rgb[n, 3]"""
    S, C = scene(u_time), constants()
    n = mat.size
    out = np.zeros((n, 3), dtype=F)
    with np.errstate(all="ignore"):
        L = C["sun_dir"]
        V = normalize(tuple(eye[k] - p[k] for k in range(3)))
        base = np.zeros((n, 3), dtype=F)
        for m_id, col in BASE_COLOR.items():
            base[mat == m_id] = col
        g = np.flatnonzero((mat == MAT_GROOVE) | (mat == MAT_DEAD_WAX))
        if g.size:                                  # :300-353
            rot = S["platter_rot"]
            ho = vec_mat(tuple(p[k][g] for k in range(3)), rot)
            Lr = vec_mat(L, rot)
            Vr = vec_mat(tuple(V[k][g] for k in range(3)), rot)
            r = length3(ho)
            B = (ho[0] / r, ho[1] / r, ho[2] / r)
            N = [np.zeros(g.size, dtype=F), np.ones(g.size, dtype=F), np.zeros(g.size, dtype=F)]
            mg = mat[g]
            is_g = mg == MAT_GROOVE
            if is_g.any():
                xyz = np.stack([ho[k] * F(2.456) for k in range(3)], axis=1)
                rr = r + F(.07575) * oracle().noise("noise_iq", xyz)[:, 0]
                s = pulse(rr * F(24.))
                k = is_g & (s > ZERO)
                Nn = normalize((N[0] + B[0], N[1] + B[1], N[2] + B[2]))
                d2 = TWO * ((ZERO * Nn[0] + ONE * Nn[1]) + ZERO * Nn[2])                  # reflect(N, (0, 1, 0)) util_optics.h:17-22
                Nr = (Nn[0] - d2 * ZERO, Nn[1] - d2 * ONE, Nn[2] - d2 * ZERO)
                for c in range(3):
                    N[c] = np.where(k, Nr[c], N[c])
            is_d = mg == MAT_DEAD_WAX
            if is_d.any():
                s = saw(r * F(4.))
                f = np.where(s > F(.9), ONE, ZERO).astype(F)
                Nd = normalize((N[0] + B[0] * f, N[1] + B[1] * f, N[2] + B[2] * f))
                for c in range(3):
                    N[c] = np.where(is_d, Nd[c], N[c])
            N = tuple(N)
            T = cross(B, N)
            ro_diff, ro_spec, a_x, a_y = F(1.), F(.0725), F(.025), F(.5)
            Hh = normalize((Vr[0] + Lr[0], Vr[1] + Lr[1], Vr[2] + Lr[2]))
            dotLN = dot(Lr, N)
            dmax = fmax(np.zeros_like(dotLN), dotLN)
            spec_a = ro_spec / np.sqrt(dotLN * dot(Vr, N))
            spec_b = ONE / (F(4.) * PI * a_x * a_y)
            ht = dot(Hh, T) / a_x
            hb = dot(Hh, B) / a_y
            spec_c = F(-2.) * (ht * ht + hb * hb) / (ONE + dot(Hh, N))
            spec = ONE * spec_a * spec_b * oracle().math("exp", spec_c)
            for c in range(3):
                out[g, c] = base[g, c] * (ro_diff / PI) * dmax + spec
        e = np.flatnonzero(~((mat == MAT_GROOVE) | (mat == MAT_DEAD_WAX)))
        if e.size:                                  # :354-378
            pe = tuple(p[k][e] for k in range(3))
            nrm = sdf_normal(build, u_time, pe)
            if build == "ridges":                   # :358-363, on the unrotated hit.origin
                me = mat[e]
                k = (me == MAT_LABEL) | (me == MAT_LOGO)
                r = length3(pe)
                B = (pe[0] / r, pe[1] / r, pe[2] / r)
                s = saw(r * F(.9))
                f = np.where(s > F(.975), ONE, ZERO).astype(F)
                nr = normalize((nrm[0] + B[0] * f, nrm[1] + B[1] * f, nrm[2] + B[2] * f))
                nrm = tuple(np.where(k, nr[c], nrm[c]) for c in range(3))
            dLn = dot(L, nrm)
            diff = fmax(np.zeros_like(dLn), dLn)
            Ve = tuple(V[k][e] for k in range(3))
            Hh = normalize((Ve[0] + L[0], Ve[1] + L[1], Ve[2] + L[2]))
            dHn = dot(Hh, nrm)
            spec = oracle().math("pow", fmax(np.zeros_like(dHn), dHn), F(50.)) * ONE
            for c in range(3):
                out[e, c] = base[e, c] * diff + spec
    return out


# ---- the pixel -----------------------------------------------------------------------------------------------------------

def render(build, u_time, ro, rd, parts=None):
    """render (:407-458) for rays (ro, rd[3][n]) -> rgb[n, 3].  parts: a dict that receives hit, p, mat, sh (the value of `sh` at
    :451: sdf_shadow's, or 1. in the build that compiles the call out) and lit (illuminate's colour)."""
    n = rd[0].size
    t = np.zeros(n, dtype=F)
    hit = np.zeros(n, dtype=bool)
    mat = np.zeros(n, dtype=np.int32)
    p = [np.zeros(n, dtype=F) for _ in range(3)]
    act = np.arange(n)
    sun = constants()["sun_dir"]
    with np.errstate(all="ignore"):
        for _ in range(STEPS):
            if act.size == 0:
                break
            ta = t[act]
            pi = tuple(ro[k] + rd[k][act] * ta for k in range(3))
            d, m = sdf(build, u_time, *pi)
            brk = ta > F(40.)
            h = ~brk & (d < F(.005))
            go = ~brk & ~h
            ih = act[h]
            hit[ih] = True
            mat[ih] = m[h].astype(np.int32)
            for k in range(3):
                p[k][ih] = pi[k][h]
            t[act[go]] = ta[go] + d[go]
            act = act[go]
        rgb = np.ones((n, 3), dtype=F)              # background :15-18
        ih = np.flatnonzero(hit)
        sh = np.ones(n, dtype=F)
        lit = np.zeros((n, 3), dtype=F)
        if ih.size:
            ph = tuple(p[k][ih] for k in range(3))
            if build != "noshadow":                 # :445-450
                sh[ih] = sdf_shadow(build, u_time, ph[0] + sun[0] * F(0.05), ph[1] + sun[1] * F(0.05), ph[2] + sun[2] * F(0.05))
            lit[ih] = illuminate(build, u_time, ro, ph, mat[ih])
            rgb[ih] = lit[ih] * sh[ih][:, None]
        if parts is not None:
            parts.update(hit=hit, p=np.stack(p, axis=1), mat=mat, sh=sh, lit=lit)
    return rgb


def main_image(build, width, height, u_time, fx, fy, parts=None):
    """fragColor at fragCoords (fx, fy) -> float32 [..., 4]"""
    assert build in BUILDS, build
    fx, fy = np.broadcast_arrays(_f(fx), _f(fy))
    shape = fx.shape
    eye, look_at = CAMERA[build]
    pcx, pcy = point_cam(width, height, fx.ravel(), fy.ravel(), FOV)
    rd = get_primary_ray(pcx, pcy, eye, look_at)
    rgb = render(build, u_time, eye, rd, parts)
    out = np.ones((fx.size, 4), dtype=F)            # main.h:52
    out[:, :3] = oracle().math("pow", np.ascontiguousarray(rgb).ravel(), F(1) / F(2.2)).reshape(rgb.shape)
    return out.reshape(shape + (4,))


def frame(build, width, height, u_time, mouse=(0.0, 0.0), parts=None):
    """float32 [H, W, 4] of the frame (row 0 = bottom; fragCoord = pixel centre).  u_mouse is not read (its only use is under SHADERTOY)."""
    fx = (np.arange(width, dtype=F) + F(.5))[None, :]
    fy = (np.arange(height, dtype=F) + F(.5))[:, None]
    return main_image(build, width, height, u_time, fx, fy, parts)


fixture = functools.partial(builds_fixture, "vinyl")     # tests/golden/vinyl_builds/ decoded: tests/model_common.py
